// tracking_layout_driver.cpp -- what the problem compiler (altro_problem.hpp: host code, no HIP) makes of tracking costs
// (altro_set_lqr_tracking_cost), printed as one JSON object {case: layout}.  tests/test_tracking_layout.py holds the
// expectations.
#include <cstdio>
#include <string>
#include <vector>

#include "altro_problem.hpp"

using namespace altro_hip;

static CostSpec Cost(int n, int m, int kb, int ke, double q, bool tracking, double xref = 1.0) {
  CostSpec c{};
  c.k_begin = kb;
  c.k_end = ke;
  c.Q.assign((size_t)n * n, 0.0);
  c.R.assign((size_t)m * m, 0.0);
  for (int i = 0; i < n; ++i) c.Q[i + i * n] = q + i;
  for (int i = 0; i < m; ++i) c.R[i + i * m] = 0.5 + i;
  c.per_instance = 0;
  c.tracking = tracking ? 1 : 0;
  if (!tracking) {
    c.xref.assign(n, xref);
    c.uref.assign(m, 0.0);
  }
  return c;
}
static void Dump(const char* name, const CompiledProblem<double>& cp, bool last = false) {
  const ProblemDesc& pd = cp.pd;
  printf("\"%s\": {\"status\": %d, \"err\": \"%s\", \"ngroups\": %d, \"nclass\": %d, \"nruns\": %d, \"npool\": %d, \"nslots\": %d, ", name,
         (int)cp.status, cp.err.c_str(), pd.ngroups, pd.nclass, pd.nruns, pd.npool, pd.nslots);
  printf("\"knot_group\": [");
  for (size_t k = 0; k < cp.knot_class.size(); ++k) printf("%s%d", k ? ", " : "", pd.cls[cp.knot_class[k]].cost_group);
  printf("], \"fast\": [");
  for (int r = 0; r < pd.nruns; ++r) printf("%s%d", r ? ", " : "", pd.runs[r].fast);
  printf("], \"groups\": [");
  for (int g = 0; g < pd.ngroups; ++g) {
    const CostGroupDesc& d = pd.grp[g];
    printf("%s{\"Q_off\": %d, \"R_off\": %d, \"q_off\": %d, \"r_off\": %d, \"c_off\": %d, \"q_pi\": %d, \"r_pi\": %d, \"c_pi\": %d, "
           "\"q_diag\": %d, \"r_diag\": %d, \"Q00\": %.17g}",
           g ? ", " : "", d.Q_off, d.R_off, d.q_off, d.r_off, d.c_off, d.q_pi, d.r_pi, d.c_pi, d.q_diag, d.r_diag, cp.pool[d.Q_off]);
  }
  printf("]}%s\n", last ? "" : ",");
}

int main() {
  const int n = 3, m = 2, N = 24;
  const UserTypeTable none;
  printf("{\n\"sizes\": {\"CostGroupDesc\": %zu, \"ProblemDesc\": %zu, \"per_knot\": %d, \"record\": %d, \"point\": %d},\n", sizeof(CostGroupDesc),
         sizeof(ProblemDesc), kParPerKnot, RefTermRecord(n, m), RefPathRecord(n, m));
  ConSpec bound{};
  bound.kind = ALTRO_CON_CONTROL_BOUND;
  bound.k_begin = 0;
  bound.k_end = N;
  bound.nparams = 4;
  bound.params = {-0.7, -0.7, 0.7, 0.7};
  {  // a reference of its own on each of the 25 knots: a stage range and the terminal knot
    ProblemSpec s;
    s.costs = {Cost(n, m, 0, N, 1.0, true), Cost(n, m, N, N + 1, 100.0, true)};
    s.cons = {bound};
    Dump("tracking_25", CompileProblem<double>(s, n, m, N, 5, none));
  }
  {  // the same written as 25 ordinary costs, one per knot, each with its own xref
    ProblemSpec s;
    for (int k = 0; k <= N; ++k) s.costs.push_back(Cost(n, m, k, k + 1, k < N ? 1.0 : 100.0, false, 0.1 * k));
    s.cons = {bound};
    Dump("ordinary_25", CompileProblem<double>(s, n, m, N, 5, none));
  }
  {  // the last cost set on a knot wins, whichever kind: tracking everywhere, then an ordinary cost on [0, 4) and, set
     // before and covered entirely, an ordinary cost on [10, 12)
    ProblemSpec s;
    s.costs = {Cost(n, m, 10, 12, 7.0, false), Cost(n, m, 0, N + 1, 1.0, true), Cost(n, m, 0, 4, 3.0, false)};
    Dump("mixed", CompileProblem<double>(s, n, m, N, 1, none), true);
  }
  printf("}\n");
  return 0;
}
