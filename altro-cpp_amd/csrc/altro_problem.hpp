// altro_problem.hpp — the problem compiler: the recorded setter calls (ProblemSpec) become the device's problem
// description (ProblemDesc: cost groups, constraint descriptors, knot classes, runs, row bases) and the two parameter pools.
// Pure host arithmetic over altro_common.hpp types: no HIP in here, so it builds and is tested with a plain C++ compiler
// (tests/test_problem_layout.py).
#pragma once

#include <cmath>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "altro_common.hpp"

namespace altro_hip {

// What the compiler needs to know of a model's user types (altro_device.hpp: UserCostList / UserConList), one entry per
// type in the order of the source's lists.  Empty: the model defines none.
struct UserTypeTable {
  std::vector<int> cost_nparams;
  std::vector<int> con_nparams, con_p, con_eq;
};

template <class T>
struct CompiledProblem {
  altro_status status = ALTRO_OK;
  std::string err;
  ProblemDesc pd{};                // everything but Bp (the padded batch is the engine's business)
  std::vector<T> pool;             // shared parameters
  std::vector<std::vector<T>> ip;  // per-instance slots, each [B]
  std::vector<int> knot_class, knot_rowbase;
  std::vector<int> con_kb, con_ke, con_p, con_eq;  // knots, rows and cone of every registered constraint (MpcRowMap)
  // knot constraints (altro_add_knot_constraint): element of every registered constraint's parameters in the knot-parameter
  // record (-1: an ordinary constraint), and the doubles of one record (their sum, rounded up to a pair; 0: none)
  std::vector<int> con_knot_off;
  int knot_record = 0;

  CompiledProblem& Fail(altro_status st, const std::string& what) {
    status = st;
    err = what;
    return *this;
  }
  // E parameters into the shared pool (returns the first element), or one slot per element per instance, v = [B][E]
  // (returns the first slot; -1 if there is none)
  template <class V>
  int Put(bool per_instance, const V& v, int E) {
    if (!per_instance) {
      const int off = (int)pool.size();
      for (int e = 0; e < E; ++e) pool.push_back(T(v[e]));
      return off;
    }
    const int B = pd.B;
    int first = -1;
    for (int e = 0; e < E; ++e) {
      ip.emplace_back(B, T(0));
      const int sl = (int)ip.size() - 1;
      if (e == 0) first = sl;
      for (int b = 0; b < B; ++b) ip[sl][b] = T(v[(size_t)b * E + e]);
    }
    return first;
  }
};

// Build the problem description of `s` for n states, m controls, N steps and B instances.
template <class T>
CompiledProblem<T> CompileProblem(const ProblemSpec& s, int n, int m, int N, int B, const UserTypeTable& user) {
  CompiledProblem<T> cp;
  ProblemDesc& pd = cp.pd;
  std::vector<T>& pool = cp.pool;
  pd.n = n;
  pd.m = m;
  pd.N = N;
  pd.B = B;

  // --- costs: the last SetCostFunction on a knot wins (problem.hpp:113-127) ---------------------
  std::vector<int> knot_cost(N + 1, -1);
  for (size_t ci = 0; ci < s.costs.size(); ++ci)
    for (int k = s.costs[ci].k_begin; k < s.costs[ci].k_end; ++k) knot_cost[k] = (int)ci;
  for (int k = 0; k <= N; ++k)
    if (knot_cost[k] < 0)
      return cp.Fail(ALTRO_NOT_READY, "cost function missing at knot " + std::to_string(k) + " (Problem::IsFullyDefined)");
  std::map<int, int> group_of_cost;
  for (int k = 0; k <= N; ++k) {
    const int ci = knot_cost[k];
    if (group_of_cost.count(ci)) continue;
    if (pd.ngroups >= kMaxCostGroups) return cp.Fail(ALTRO_UNSUPPORTED, "too many distinct cost functions");
    const CostSpec& c = s.costs[ci];
    CostGroupDesc g{};
    if (c.user) {
      // the user model's UserCost (altro_set_user_cost): only its parameters travel
      if (user.cost_nparams.empty())
        return cp.Fail(ALTRO_INVALID_ARG,
                       "this model defines no UserCost (altro_set_user_cost needs a user model whose source defines ALTRO_USER_COST)");
      if (c.user - 1 < 0 || c.user - 1 >= (int)user.cost_nparams.size())
        return cp.Fail(ALTRO_INVALID_ARG, "user cost type " + std::to_string(c.user - 1) + ": the model's source defines " +
                                              std::to_string(user.cost_nparams.size()) + " cost type(s) (ALTRO_USER_COSTS)");
      const int NP = user.cost_nparams[c.user - 1];
      if ((int)c.params.size() != NP * (c.per_instance ? B : 1))
        return cp.Fail(ALTRO_INVALID_ARG, "user cost type " + std::to_string(c.user - 1) + ": expected " + std::to_string(NP) +
                                              " parameters" + (c.per_instance ? " per instance" : ""));
      g.user = c.user;
      g.u_pi = c.per_instance ? 1 : 0;
      // (the quadratic fields stay valid, all-zero pool entries: every generic read is in bounds)
      g.Q_off = g.R_off = g.q_off = g.r_off = g.c_off = (int)pool.size();
      for (int e = 0; e < n * n + m * m; ++e) pool.push_back(T(0));
      g.u_off = cp.Put(g.u_pi != 0, c.params, NP);
      if (g.u_off < 0) g.u_off = (int)cp.ip.size();  // (a per-instance type without parameters: where its slots would start)
      group_of_cost[ci] = pd.ngroups;
      pd.grp[pd.ngroups++] = g;
      continue;
    }
    // QuadraticCost::LQRCost (examples/quadratic_cost.hpp:29-39), evaluated in T like the oracle
    g.Q_off = (int)pool.size();
    for (int e = 0; e < n * n; ++e) pool.push_back(T(c.Q[e]));
    g.R_off = (int)pool.size();
    for (int e = 0; e < m * m; ++e) pool.push_back(T(c.R[e]));
    const std::vector<T> Q(pool.begin() + g.Q_off, pool.begin() + g.Q_off + n * n);
    const std::vector<T> R(pool.begin() + g.R_off, pool.begin() + g.R_off + m * m);
    g.q_diag = g.r_diag = 1;
    for (int j = 0; j < n; ++j)
      for (int i = 0; i < n; ++i)
        if (i != j && Q[i + j * n] != T(0)) g.q_diag = 0;
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < m; ++i)
        if (i != j && R[i + j * m] != T(0)) g.r_diag = 0;
    if (c.tracking) {
      // LQRCost(Q, R, xref_k, uref_k) with the handle's reference at every knot (altro_set_lqr_tracking_cost): the terms
      // live in the reference-term records, which k_ref_terms fills -- element q_off / r_off / c_off of the knot's record
      g.q_pi = g.r_pi = g.c_pi = kParPerKnot;
      g.q_off = 0;
      g.r_off = n;
      g.c_off = n + m;
      group_of_cost[ci] = pd.ngroups;
      pd.grp[pd.ngroups++] = g;
      continue;
    }
    const bool xpi = (c.per_instance & 1) != 0, upi = (c.per_instance & 2) != 0;
    g.q_pi = xpi;
    g.r_pi = upi;
    g.c_pi = xpi || upi;
    const int ninst_q = xpi ? B : 1, ninst_r = upi ? B : 1, ninst_c = g.c_pi ? B : 1;
    std::vector<T> q((size_t)ninst_q * n), r((size_t)ninst_r * m), cc(ninst_c);
    std::vector<T> xQx(ninst_q), uRu(ninst_r);
    // v = -W ref per instance, and ref' W ref
    auto linear_term = [](const std::vector<T>& W, const std::vector<double>& ref, int E, int ninst, std::vector<T>& v,
                          std::vector<T>& rWr) {
      std::vector<T> xr(E), Wx(E);
      for (int b = 0; b < ninst; ++b) {
        for (int i = 0; i < E; ++i) xr[i] = T(ref[(size_t)b * E + i]);
        T acc = T(0);
        for (int i = 0; i < E; ++i) {
          T sacc = T(0);
          for (int j = 0; j < E; ++j) sacc += W[i + j * E] * xr[j];
          Wx[i] = sacc;
          v[(size_t)b * E + i] = -sacc;
        }
        for (int i = 0; i < E; ++i) acc += xr[i] * Wx[i];
        rWr[b] = acc;
      }
    };
    linear_term(Q, c.xref, n, ninst_q, q, xQx);
    linear_term(R, c.uref, m, ninst_r, r, uRu);
    for (int b = 0; b < ninst_c; ++b) cc[b] = T(0.5) * xQx[xpi ? b : 0] + T(0.5) * uRu[upi ? b : 0];
    g.q_off = cp.Put(xpi, q, n);
    g.r_off = cp.Put(upi, r, m);
    g.c_off = cp.Put(g.c_pi != 0, cc, 1);
    group_of_cost[ci] = pd.ngroups;
    pd.grp[pd.ngroups++] = g;
  }

  // --- constraints: per knot, equalities first then inequalities, insertion order kept ----------
  std::vector<ConDesc> built(s.cons.size());
  cp.con_knot_off.assign(s.cons.size(), -1);
  int nknot = 0;
  for (size_t i = 0; i < s.cons.size(); ++i) {
    const ConSpec& c = s.cons[i];
    ConDesc d{};
    d.kind = c.kind;
    d.per_instance = c.knot ? kParPerKnotCon : (c.per_instance ? 1 : 0);
    if (c.kind == ALTRO_CON_GOAL) {
      if (c.nparams != n) return cp.Fail(ALTRO_INVALID_ARG, "goal constraint needs n parameters");
      d.type = 0;
      d.p = n;
    } else if (c.kind == ALTRO_CON_CONTROL_BOUND) {
      if (c.nparams != 2 * m || (c.per_instance && !c.knot)) return cp.Fail(ALTRO_INVALID_ARG, "control bound needs 2m shared parameters");
      d.type = 1;
      for (int j = 0; j < m; ++j) {  // GetFiniteIndices, basic_constraints.hpp:138-145
        // (a knot bound: every entry of its track is finite -- the setters refuse anything else -- so it has all 2m rows)
        if (c.knot || std::abs(c.params[j]) < std::numeric_limits<double>::max()) d.lo_mask |= 1u << j;
        if (c.knot || std::abs(c.params[m + j]) < std::numeric_limits<double>::max()) d.hi_mask |= 1u << j;
      }
      d.p = __builtin_popcount(d.lo_mask) + __builtin_popcount(d.hi_mask);
    } else if (c.kind == ALTRO_CON_CIRCLE) {
      if (c.nparams % 3 != 0 || c.nparams == 0 || n < 2)
        return cp.Fail(ALTRO_INVALID_ARG, "circle constraint needs (cx, cy, r) triples");
      d.type = 1;
      d.p = c.nparams / 3;
    } else if (c.kind == ALTRO_CON_USER) {
      // the user model's UserConstraint: OutputDimension and cone come from its source
      if (user.con_nparams.empty())
        return cp.Fail(ALTRO_INVALID_ARG,
                       "this model defines no UserConstraint (ALTRO_CON_USER needs a user model whose source defines ALTRO_USER_CONSTRAINT)");
      if (c.user_type < 0 || c.user_type >= (int)user.con_nparams.size())
        return cp.Fail(ALTRO_INVALID_ARG, "user constraint type " + std::to_string(c.user_type) + ": the model's source defines " +
                                              std::to_string(user.con_nparams.size()) + " constraint type(s) (ALTRO_USER_CONSTRAINTS)");
      const int unp = user.con_nparams[c.user_type];
      if (c.nparams != unp)
        return cp.Fail(ALTRO_INVALID_ARG,
                       "user constraint type " + std::to_string(c.user_type) + ": expected " + std::to_string(unp) + " parameters");
      d.type = user.con_eq[c.user_type] ? 0 : 1;
      d.p = user.con_p[c.user_type];
      d.lo_mask = (unsigned)c.user_type;  // (the device dispatches on it: user_con_auglag)
    } else {
      return cp.Fail(ALTRO_INVALID_ARG, "unknown constraint kind");
    }
    if (c.knot) {
      // the parameters live in the knot-parameter records, which k_knot_params fills from the constraint's track
      if (nknot >= kMaxKnotCons) return cp.Fail(ALTRO_UNSUPPORTED, "too many knot constraints");
      ++nknot;
      d.param_off = cp.knot_record;
      cp.con_knot_off[i] = cp.knot_record;
      cp.knot_record += c.nparams;
    } else if (d.kind == ALTRO_CON_CONTROL_BOUND) {
      d.param_off = (int)pool.size();
      for (int j = 0; j < m; ++j)
        if ((d.lo_mask >> j) & 1u) pool.push_back(T(c.params[j]));
      for (int j = 0; j < m; ++j)
        if ((d.hi_mask >> j) & 1u) pool.push_back(T(c.params[m + j]));
    } else {
      d.param_off = cp.Put(d.per_instance != 0, c.params, c.nparams);
    }
    built[i] = d;
  }
  cp.knot_record = (cp.knot_record + 1) & ~1;
  for (size_t i = 0; i < s.cons.size(); ++i) {  // (what the row map of a receding-horizon advance is built from: MpcRowMap)
    cp.con_kb.push_back(s.cons[i].k_begin);
    cp.con_ke.push_back(s.cons[i].k_end);
    cp.con_p.push_back(built[i].p);
    cp.con_eq.push_back(built[i].type == 0 ? 1 : 0);
  }
  std::vector<std::vector<int>> knot_cons(N + 1);
  for (size_t i = 0; i < s.cons.size(); ++i)
    for (int k = s.cons[i].k_begin; k < s.cons[i].k_end; ++k) knot_cons[k].push_back((int)i);
  for (auto& v : knot_cons) std::stable_partition(v.begin(), v.end(), [&](int i) { return built[i].type == 0; });

  // --- knot classes --------------------------------------------------------------------------------
  std::map<std::vector<int>, int> class_of;
  cp.knot_class.assign(N + 1, 0);
  cp.knot_rowbase.assign(N + 1, 0);
  int rows = 0;
  for (int k = 0; k <= N; ++k) {
    std::vector<int> key;
    key.push_back(group_of_cost[knot_cost[k]]);
    for (int i : knot_cons[k]) key.push_back(i);
    auto it = class_of.find(key);
    int cls;
    if (it == class_of.end()) {
      if (pd.nclass >= kMaxClasses) return cp.Fail(ALTRO_UNSUPPORTED, "too many distinct knot-point classes");
      if ((int)knot_cons[k].size() > kMaxConPerKnot) return cp.Fail(ALTRO_UNSUPPORTED, "too many constraints on one knot point");
      cls = pd.nclass++;
      KnotClass& kc = pd.cls[cls];
      kc.cost_group = key[0];
      kc.ncon = (int)knot_cons[k].size();
      int ro = 0;
      for (int c = 0; c < kc.ncon; ++c) {
        kc.con[c] = built[knot_cons[k][c]];
        kc.con[c].row_off = ro;
        ro += kc.con[c].p;
      }
      kc.nrows = ro;
      class_of[key] = cls;
    } else {
      cls = it->second;
    }
    cp.knot_class[k] = cls;
    cp.knot_rowbase[k] = rows;
    rows += pd.cls[cls].nrows;
  }
  pd.total_rows = rows;
  pd.nslots = (int)cp.ip.size();
  pd.npool = (int)pool.size();
  pd.hstep = s.hstep;
  // runs of consecutive knots sharing a class (scalar-register friendly serial loops)
  pd.nruns = 0;
  for (int k = 0; k <= N; ++k) {
    if (pd.nruns > 0 && pd.runs[pd.nruns - 1].cls == cp.knot_class[k]) {
      pd.runs[pd.nruns - 1].k_end = k + 1;
      continue;
    }
    if (pd.nruns >= kMaxRuns) return cp.Fail(ALTRO_UNSUPPORTED, "too many runs of distinct knot-point classes");
    KnotRun run{};
    run.k_begin = k;
    run.k_end = k + 1;
    run.cls = cp.knot_class[k];
    run.rowbase = cp.knot_rowbase[k];
    const KnotClass& kc = pd.cls[run.cls];
    const unsigned full = (1u << m) - 1u;
    auto is_full_bound = [&](const ConDesc& c) { return c.kind == ALTRO_CON_CONTROL_BOUND && c.lo_mask == full && c.hi_mask == full; };
    auto is_circle = [&](const ConDesc& c) { return c.kind == ALTRO_CON_CIRCLE && c.p <= kMaxFastCircles; };  // (cost_consumer_run keeps them in registers)
    run.fast = kFastGeneric;
    if (pd.grp[kc.cost_group].q_diag && pd.grp[kc.cost_group].r_diag) {
      if (kc.ncon == 0) run.fast = kFastNone;
      else if (kc.ncon == 1 && is_full_bound(kc.con[0])) run.fast = kFastB;
      else if (kc.ncon == 1 && is_circle(kc.con[0])) run.fast = kFastC;
      else if (kc.ncon == 2 && is_circle(kc.con[0]) && is_full_bound(kc.con[1])) run.fast = kFastCB;
      else if (kc.ncon == 2 && is_full_bound(kc.con[0]) && is_circle(kc.con[1])) run.fast = kFastBC;
    }
    pd.runs[pd.nruns++] = run;
  }
  return cp;
}

}  // namespace altro_hip
