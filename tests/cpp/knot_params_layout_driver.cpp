// knot_params_layout_driver.cpp -- what the problem compiler (altro_problem.hpp: host code, no HIP) makes of knot constraints
// (altro_add_knot_constraint, include/altro_knot_params.h), printed as one JSON object {case: layout}.
// tests/test_knot_params_layout.py holds the expectations.
#include <cstdio>
#include <string>
#include <vector>

#include "altro_problem.hpp"

using namespace altro_hip;

static CostSpec Tracking(int n, int m, int kb, int ke, double q) {
  CostSpec c{};
  c.k_begin = kb;
  c.k_end = ke;
  c.Q.assign((size_t)n * n, 0.0);
  c.R.assign((size_t)m * m, 0.0);
  for (int i = 0; i < n; ++i) c.Q[i + i * n] = q + i;
  for (int i = 0; i < m; ++i) c.R[i + i * m] = 0.5 + i;
  c.per_instance = 0;
  c.tracking = 1;
  return c;
}
static ConSpec Con(int kind, int kb, int ke, int np, bool knot, std::vector<double> params = {}) {
  ConSpec c{};
  c.kind = kind;
  c.k_begin = kb;
  c.k_end = ke;
  c.nparams = np;
  c.per_instance = 0;
  c.knot = knot ? 1 : 0;
  c.params = std::move(params);
  return c;
}
static void Dump(const char* name, const CompiledProblem<double>& cp, bool last = false) {
  const ProblemDesc& pd = cp.pd;
  printf("\"%s\": {\"status\": %d, \"err\": \"%s\", \"nclass\": %d, \"nruns\": %d, \"npool\": %d, \"nslots\": %d, \"total_rows\": %d, "
         "\"knot_record\": %d, ",
         name, (int)cp.status, cp.err.c_str(), pd.nclass, pd.nruns, pd.npool, pd.nslots, pd.total_rows, cp.knot_record);
  printf("\"knot_class\": [");
  for (size_t k = 0; k < cp.knot_class.size(); ++k) printf("%s%d", k ? ", " : "", cp.knot_class[k]);
  printf("], \"con_knot_off\": [");
  for (size_t i = 0; i < cp.con_knot_off.size(); ++i) printf("%s%d", i ? ", " : "", cp.con_knot_off[i]);
  printf("], \"con_p\": [");
  for (size_t i = 0; i < cp.con_p.size(); ++i) printf("%s%d", i ? ", " : "", cp.con_p[i]);
  printf("], \"runs\": [");
  for (int r = 0; r < pd.nruns; ++r)
    printf("%s{\"k_begin\": %d, \"k_end\": %d, \"cls\": %d, \"fast\": %d}", r ? ", " : "", pd.runs[r].k_begin, pd.runs[r].k_end, pd.runs[r].cls,
           pd.runs[r].fast);
  printf("], \"classes\": [");
  for (int c = 0; c < pd.nclass; ++c) {
    const KnotClass& kc = pd.cls[c];
    printf("%s{\"nrows\": %d, \"cons\": [", c ? ", " : "", kc.nrows);
    for (int i = 0; i < kc.ncon; ++i)
      printf("%s{\"kind\": %d, \"p\": %d, \"per_instance\": %d, \"param_off\": %d, \"row_off\": %d, \"lo_mask\": %u, \"hi_mask\": %u}", i ? ", " : "",
             kc.con[i].kind, kc.con[i].p, kc.con[i].per_instance, kc.con[i].param_off, kc.con[i].row_off, kc.con[i].lo_mask, kc.con[i].hi_mask);
    printf("]}");
  }
  printf("]}%s\n", last ? "" : ",");
}

int main() {
  const int n = 3, m = 2, N = 24;
  const UserTypeTable none;
  printf("{\n\"sizes\": {\"ProblemDesc\": %zu, \"KnotClass\": %zu, \"ConDesc\": %zu, \"marker\": %d, \"max_knot_cons\": %d},\n", sizeof(ProblemDesc),
         sizeof(KnotClass), sizeof(ConDesc), kParPerKnotCon, kMaxKnotCons);
  const std::vector<CostSpec> costs = {Tracking(n, m, 0, N, 1.0), Tracking(n, m, N, N + 1, 100.0)};
  {  // problems.moving_obstacles: two moving circles on [1, N), then a control bound on [0, N), both knot constraints
    ProblemSpec s;
    s.costs = costs;
    s.cons = {Con(ALTRO_CON_CIRCLE, 1, N, 6, true), Con(ALTRO_CON_CONTROL_BOUND, 0, N, 4, true)};
    Dump("moving_obstacles", CompileProblem<double>(s, n, m, N, 5, none));
  }
  {  // the same written as one ordinary constraint per knot, each with parameters of its own
    ProblemSpec s;
    s.costs = costs;
    for (int k = 0; k < N; ++k) {
      if (k >= 1) s.cons.push_back(Con(ALTRO_CON_CIRCLE, k, k + 1, 6, false, {1.0, 0.5 - 0.01 * k, 0.1, 0.1 * k, -0.3, 0.15}));
      s.cons.push_back(Con(ALTRO_CON_CONTROL_BOUND, k, k + 1, 4, false, {-0.9 + 0.008 * k, -0.9 + 0.008 * k, 0.9 - 0.008 * k, 0.9 - 0.008 * k}));
    }
    Dump("ordinary_per_knot", CompileProblem<double>(s, n, m, N, 5, none));
  }
  {  // a knot goal on the terminal knot beside an ordinary shared circle and a knot bound: the ordinary one keeps its pool
    ProblemSpec s;
    s.costs = costs;
    s.cons = {Con(ALTRO_CON_CONTROL_BOUND, 0, N, 4, true), Con(ALTRO_CON_CIRCLE, 1, N, 3, false, {1.0, 0.5, 0.1}),
              Con(ALTRO_CON_GOAL, N, N + 1, 3, true)};
    Dump("mixed", CompileProblem<double>(s, n, m, N, 5, none));
  }
  {  // a knot constraint whose nparams does not fit its kind
    ProblemSpec s;
    s.costs = costs;
    s.cons = {Con(ALTRO_CON_CONTROL_BOUND, 0, N, 3, true)};
    Dump("bad_nparams", CompileProblem<double>(s, n, m, N, 5, none), true);
  }
  printf("}\n");
  return 0;
}
