// problem_layout_driver.cpp -- builds small ProblemSpecs, runs the problem compiler (altro_problem.hpp: host code, no HIP)
// and prints what it produced as one JSON object {case: layout}.  tests/test_problem_layout.py holds the expectations.
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "altro_problem.hpp"

using namespace altro_hip;

static std::vector<double> Diag(int n, double v) {
  std::vector<double> M((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) M[i + i * n] = v + i;
  return M;
}
static CostSpec Lqr(int n, int m, int kb, int ke, double q) {
  CostSpec c{};
  c.k_begin = kb;
  c.k_end = ke;
  c.Q = Diag(n, q);
  c.R = Diag(m, 0.5);
  c.xref.assign(n, 1.0);
  c.uref.assign(m, 0.0);
  c.per_instance = 0;
  return c;
}
static ConSpec Con(int kind, int kb, int ke, std::vector<double> params, int nparams, int per_instance = 0) {
  ConSpec c{};
  c.kind = kind;
  c.k_begin = kb;
  c.k_end = ke;
  c.nparams = nparams;
  c.per_instance = per_instance;
  c.params = std::move(params);
  return c;
}

template <class V>
static void List(const char* name, const V& v, bool last = false) {
  printf("\"%s\": [", name);
  for (size_t i = 0; i < v.size(); ++i) printf("%s%.17g", i ? ", " : "", (double)v[i]);
  printf("]%s", last ? "" : ", ");
}
static void Dump(const char* name, const CompiledProblem<double>& cp, bool last = false) {
  const ProblemDesc& pd = cp.pd;
  printf("\"%s\": {\"status\": %d, \"err\": \"%s\", ", name, (int)cp.status, cp.err.c_str());
  printf("\"ngroups\": %d, \"nclass\": %d, \"nruns\": %d, \"total_rows\": %d, \"nslots\": %d, \"npool\": %d, ", pd.ngroups, pd.nclass,
         pd.nruns, pd.total_rows, pd.nslots, pd.npool);
  List("pool", cp.pool);
  List("knot_class", cp.knot_class);
  List("knot_rowbase", cp.knot_rowbase);
  List("con_kb", cp.con_kb);
  List("con_ke", cp.con_ke);
  List("con_p", cp.con_p);
  List("con_eq", cp.con_eq);
  printf("\"slots\": [");
  for (size_t s = 0; s < cp.ip.size(); ++s) {
    printf("%s[", s ? ", " : "");
    for (size_t b = 0; b < cp.ip[s].size(); ++b) printf("%s%.17g", b ? ", " : "", cp.ip[s][b]);
    printf("]");
  }
  printf("], \"groups\": [");
  for (int g = 0; g < pd.ngroups; ++g)
    printf("%s{\"Q_off\": %d, \"q_diag\": %d, \"r_diag\": %d, \"user\": %d}", g ? ", " : "", pd.grp[g].Q_off, pd.grp[g].q_diag,
           pd.grp[g].r_diag, pd.grp[g].user);
  printf("], \"runs\": [");
  for (int r = 0; r < pd.nruns; ++r)
    printf("%s{\"k_begin\": %d, \"k_end\": %d, \"cls\": %d, \"rowbase\": %d, \"fast\": %d}", r ? ", " : "", pd.runs[r].k_begin,
           pd.runs[r].k_end, pd.runs[r].cls, pd.runs[r].rowbase, pd.runs[r].fast);
  printf("], \"classes\": [");
  for (int c = 0; c < pd.nclass; ++c) {
    const KnotClass& kc = pd.cls[c];
    printf("%s{\"cost_group\": %d, \"nrows\": %d, \"cons\": [", c ? ", " : "", kc.cost_group, kc.nrows);
    for (int j = 0; j < kc.ncon; ++j)
      printf("%s{\"kind\": %d, \"type\": %d, \"p\": %d, \"per_instance\": %d, \"param_off\": %d, \"row_off\": %d, \"lo_mask\": %u, \"hi_mask\": %u}",
             j ? ", " : "", kc.con[j].kind, kc.con[j].type, kc.con[j].p, kc.con[j].per_instance, kc.con[j].param_off, kc.con[j].row_off,
             kc.con[j].lo_mask, kc.con[j].hi_mask);
    printf("]}");
  }
  printf("]}%s\n", last ? "" : ",");
}

int main() {
  const int n = 3, m = 2, N = 8;
  const double inf = std::numeric_limits<double>::max();
  const UserTypeTable none;
  printf("{\n");
  {  // the unicycle turn: LQR stage and terminal costs, a full control bound on the stage knots, a goal at the end
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N, 1.0), Lqr(n, m, N, N + 1, 100.0)};
    s.cons = {Con(ALTRO_CON_CONTROL_BOUND, 0, N, {-1.5, -2.5, 1.5, 2.5}, 4), Con(ALTRO_CON_GOAL, N, N + 1, {1.0, 2.0, 3.0}, 3)};
    Dump("unicycle_turn", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {  // the second cost covers every knot of the first and more: the first is never counted
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, 4, 7.0), Lqr(n, m, 0, N, 1.0), Lqr(n, m, N, N + 1, 100.0)};
    Dump("last_cost_wins", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {  // ... and overlapping only partly: both stay, the later one's group on the shared knots
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N + 1, 7.0), Lqr(n, m, 2, 5, 1.0)};
    Dump("last_cost_wins_partly", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {  // an inequality added before an equality on the same knot
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N + 1, 1.0)};
    s.cons = {Con(ALTRO_CON_CONTROL_BOUND, 2, 6, {-1.5, -2.5, 1.5, 2.5}, 4), Con(ALTRO_CON_GOAL, 4, 5, {1.0, 2.0, 3.0}, 3)};
    Dump("row_order", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {  // one infinite bound: the upper bound of control 0
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N + 1, 1.0)};
    s.cons = {Con(ALTRO_CON_CONTROL_BOUND, 0, N, {-1.5, -2.5, inf, 2.5}, 4)};
    Dump("infinite_bound", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {  // one off-diagonal entry of Q
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N + 1, 1.0)};
    s.costs[0].Q[1 + 0 * n] = 0.25;
    Dump("off_diagonal", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {  // a goal of its own per instance, three instances: params [B][n]
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N + 1, 1.0)};
    s.cons = {Con(ALTRO_CON_GOAL, N, N + 1, {11, 12, 13, 21, 22, 23, 31, 32, 33}, 3, 1)};
    Dump("per_instance_goal", CompileProblem<double>(s, n, m, N, 3, none));
  }
  {  // refusals
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, 5, 1.0), Lqr(n, m, 6, N + 1, 1.0)};
    Dump("no_cost_at_knot_5", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {  // kMaxClasses + 1 classes: every knot its own goal (N + 1 = 9 knots)
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N + 1, 1.0)};
    for (int k = 0; k <= kMaxClasses; ++k) s.cons.push_back(Con(ALTRO_CON_GOAL, k, k + 1, {1.0, 2.0, 3.0}, 3));
    Dump("too_many_classes", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N + 1, 1.0)};
    s.cons = {Con(ALTRO_CON_GOAL, N, N + 1, {1.0, 2.0}, 2)};
    Dump("goal_with_two_parameters", CompileProblem<double>(s, n, m, N, 1, none));
  }
  {
    ProblemSpec s;
    s.costs = {Lqr(n, m, 0, N + 1, 1.0)};
    s.costs[0].user = 1;
    s.costs[0].params = {1.0};
    Dump("user_cost_without_user_types", CompileProblem<double>(s, n, m, N, 1, none), true);
  }
  printf("}\n");
  return 0;
}
