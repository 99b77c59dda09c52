// piadmm_obca_edge.hip -- OBCA-ADMM edge (RSU) step: batched SQP, one wavefront per slot problem,
// with lambda_update fused behind the solve (gfx950).
//
// The reference's edge NLP on the consensus variable Z (Distributed_planner/decentralized/
// optimizer.py:239-328) is separable over the 7 horizon slots: the constraints (:264-283) touch
// one slot each and the objective (:298-307) is a sum over slots.  One vehicle pair is 7
// problems in z = [s_0 (5), mu_0 (4), s_1 (5), mu_1 (4)], w = [local_x, lamb_ij]:
//     min  -z.lamb_bar + rho/2 |w - z|^2
//     s.t. g_eq = A(s_0)' mu_0 + A(s_1)' mu_1 = 0
//          min_dis <= g_in = -b(s_0)' mu_0 - b(s_1)' mu_1 <= g_max
//          |s| <= x_bound, 0 <= mu <= mu_max       (the intent of :285-295)
// The SQP ("The edge step"; tests/_obca_edge_ref.py is the same statement
// in NumPy):
//   * exact Lagrangian Hessian rho I - y_eq . Hess g_eq - y_in Hess g_in (two 9 x 9 blocks);
//   * Hessian modification: sigma * sum a a' over the equality rows and the rows active in the
//     previous QP, then tau diag(|H_ii|), until the Cholesky factorisation succeeds;
//   * the 18-variable QP (2 equalities, 38 inequality rows) by the Goldfarb-Idnani dual active
//     set method, equalities first, then the most violated row;
//   * l1-merit Armijo backtracking; multipliers blended by the step length.
//
// Layout: one wave = one slot problem, EW waves per workgroup, each wave on its own slice of LDS
// (sizeof(Es) per wave); lane i < 18 owns row / element i.  Waves never cooperate: there is no
// workgroup barrier, and a wave past the end of the batch exits whole at the top.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <string>

#include "pd_obca.h"
#include "piadmm.h"
#include "piadmm_obca_handle.h"

namespace obca_edge {

using namespace pd_obca;     // NT, the constants, the layouts, the reductions, Geo, the QP core
constexpr int NE = 18, NEP = NE + 1, NROW = 2 + 2 * NE, NEQ = 2;
constexpr int EW = 4;                          // waves (slot problems) per workgroup
constexpr int REC = PIADMM_OBCA_EDGE_REC, OUT = PIADMM_OBCA_EDGE_OUT;

constexpr double TOL_STEP = 1e-9, TOL_FEAS = 1e-9, ARMIJO = 1e-4;
constexpr int MAX_HALVINGS = 30;

struct Es {
  double H0[NE][NEP];       // the Lagrangian Hessian
  double Hm[NE][NEP];       // modified Hessian, then its Cholesky factor
  double J[NE][NEP];        // J = L^-T Q
  double R[NE][NEP];        // Ga during the modification, then R
  double Jeq[NEQ][NE], gin[NE];
  double w[NE], lb[NE], lo[NE], hi[NE];
  double z[NE], zn[NE], gf[NE], gm[NE];
  double x[NE], d[NE], npv[NE], dd[NE], u[NE + 1];
  double din[NROW], uin[NROW];
  double deq[NEQ], sgn[NEQ], ueq[NEQ];
  int act[NE + 1], pact[NROW];
  int nact, npact;
};
static_assert(EW * sizeof(Es) <= 160 * 1024 / 2, "OBCA edge workspace: two workgroups per CU");

// The wave's own LDS slice is shared among its 64 lanes only: LDS operations of one wave execute
// in order, so a compiler-level fence is what a write -> read by another lane needs.
#define WSYNC() do { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); __builtin_amdgcn_wave_barrier(); } while (0)

// this vehicle's term of g_in: -b(s)' mu
__device__ __forceinline__ double ga_val(const Geo& G, const double* Lt) {
  return -(LENGTH / 2 * Lt[0] + WIDTH / 2 * Lt[1] + LENGTH / 2 * Lt[2] + WIDTH / 2 * Lt[3]) - dot2(G.q, G.m);
}

// g_eq (2), g_in, the l1 violation and the cost at the point zz (LDS, 18); uniform results.
// Lane l evaluates the geometry of vehicle (l >= 9); lanes 0 and 9 carry the two terms.
__device__ void point_eval(const Es& S, const double* zz, int prob, double sigd, double rho, double min_dis,
                           double g_max, double g_eq[2], double& g_in, double& viol, double& cost) {
  const int lane = threadIdx.x & 63;
  const int vb = (lane >= 9 && lane < NE) ? 9 : 0;
  Geo G;
  geo(zz + vb, zz + vb + 5, prob, sigd, G);
  const double ga = ga_val(G, zz + vb + 5);
  g_eq[0] = __shfl(G.m[0], 0, 64) + __shfl(G.m[0], 9, 64);
  g_eq[1] = __shfl(G.m[1], 0, 64) + __shfl(G.m[1], 9, 64);
  g_in = __shfl(ga, 0, 64) + __shfl(ga, 9, 64);
  double bv = 0.0, cv = 0.0;
  if (lane < NE) {
    const double zl = zz[lane], dw = S.w[lane] - zl;
    bv = fmax(0.0, S.lo[lane] - zl) + fmax(0.0, zl - S.hi[lane]);
    cv = -zl * S.lb[lane] + 0.5 * rho * dw * dw;
  }
  viol = fabs(g_eq[0]) + fabs(g_eq[1]) + fmax(0.0, min_dis - g_in) + fmax(0.0, g_in - g_max) + wsum(bv);
  cost = wsum(cv);
}

// inequality row c of C d >= din: 0 / 1 the range row (+gin / -gin), then per variable j the
// lower (2 + 2j: +e_j) and upper (3 + 2j: -e_j) bound
__device__ __forceinline__ double row_elem(const Es& S, int c, int k) {
  if (c < 2) return c ? -S.gin[k] : S.gin[k];
  const int j = (c - 2) >> 1;
  return (k == j) ? ((c & 1) ? -1.0 : 1.0) : 0.0;
}
__device__ __forceinline__ double row_dot(const Es& S, int c, const double* v) {
  if (c < 2) {
    double s = 0.0;
    for (int k = 0; k < NE; ++k) s += S.gin[k] * v[k];
    return c ? -s : s;
  }
  const int j = (c - 2) >> 1;
  return (c & 1) ? -v[j] : v[j];
}
// constraint id p of the active set: p < 2 the (sign-normalised) equality p, else inequality p - 2
__device__ __forceinline__ double con_elem(const Es& S, int p, int k) {
  return (p < NEQ) ? S.Jeq[p][k] * S.sgn[p] : row_elem(S, p - NEQ, k);
}
__device__ __forceinline__ double con_rhs(const Es& S, int p) {
  return (p < NEQ) ? S.deq[p] * S.sgn[p] : S.din[p - NEQ];
}

// ---------------------------------------------------------------------------------------------
// The QP as pd_obca.h's active-set core sees it: gi_drop, gi_add and the opening and closing of
// gi_solve are stated there; the equalities are seeded here.
// ---------------------------------------------------------------------------------------------
struct QP {
  using State = Es;
  static constexpr int N = NE, NP = NEP, NEQ = obca_edge::NEQ, NROW = obca_edge::NROW;
  static __device__ __forceinline__ int lane() { return threadIdx.x & 63; }
  static __device__ __forceinline__ void fence() { WSYNC(); }
  static __device__ __forceinline__ double elem(const Es& S, int p, int k) { return con_elem(S, p, k); }
  static __device__ __forceinline__ double rhs(const Es& S, int p) { return con_rhs(S, p); }
};
// false if a pivot is not positive
__device__ __forceinline__ bool chol(double (*M)[NEP]) { return chol_n<QP>(M, NE, 0.0); }

// min 1/2 d'Hd + gm'd, Jeq d = deq, C d >= din; H = L L' in S.Hm.  0 ok, 2 infeasible, 1 step
// limit; S.x = solution, S.ueq / S.uin = multipliers.
__device__ int gi_solve(Es& S, int& steps) {
  const int lane = threadIdx.x & 63;
  gi_factor<QP>(S, S.gm);
  gi_start<QP>(S);
  for (int k = 0; k < NEQ; ++k) {
    double s = 0.0;
    for (int i = 0; i < NE; ++i) s += S.Jeq[k][i] * S.x[i];
    WSYNC();
    if (lane == 0) S.sgn[k] = (s - S.deq[k] > 0.0) ? -1.0 : 1.0;
    WSYNC();
    int ok = gi_add<QP>(S, k, steps);
    if (ok < 0) return 1;
    if (ok == 0) return 2;
  }
  while (true) {
    double best = INFINITY;
    int bi = -1;
    if (lane < NROW) {
      best = row_dot(S, lane, S.x) - S.din[lane];
      bi = lane;
    }
    wargmin(best, bi);
    if (!(best < -1e-11 * (1.0 + fabs(S.din[bi])))) break;
    int ok = gi_add<QP>(S, NEQ + bi, steps);
    if (ok < 0) return 1;
    if (ok == 0) return 2;
  }
  gi_multipliers<QP>(S);
  return 0;
}

// np.around(x, d) = rint(x 10^d) / 10^d, the rule of the QP path's round_decimals; d < 0: off
__device__ __forceinline__ double around(double x, int d) {
  if (d < 0) return x;
  double f = 1.0;
  for (int i = 0; i < d; ++i) f *= 10.0;
  return rint(x * f) / f;
}

// ---------------------------------------------------------------------------------------------
// one slot problem on this wave
// ---------------------------------------------------------------------------------------------
__device__ void edge_one(Es& S, int pair, int t, const double* __restrict__ recs, double* __restrict__ out,
                         int* __restrict__ ist) {
  const int lane = threadIdx.x & 63;
  const double* rec = recs + (size_t)pair * REC;
  const double* par = rec + E_PAR;
  const double rho = par[0], min_dis = par[1], g_max = par[8];
  const int prob = (int)par[2], max_iter = (int)par[3], rdec = (int)par[4], start = (int)par[5];
  const double x_bound = par[6], mu_max = par[7];
  const double sigd = sqrt(0.95 / (1.0 - 0.95));
  const int veh = (lane < NE && lane >= 9) ? 1 : 0, li = (lane < NE) ? lane - 9 * veh : 0;
  if (lane < NE) {
    const double wl = (li < 5) ? rec[E_LX + (veh * NT + t) * 5 + li] : rec[E_LIJ + (veh * NT + t) * 4 + (li - 5)];
    const double lo = (li < 5) ? -x_bound : 0.0, hi = (li < 5) ? x_bound : mu_max;
    S.w[lane] = wl;
    S.lb[lane] = rec[E_LB + (veh * NT + t) * 9 + li];
    S.lo[lane] = lo;
    S.hi[lane] = hi;
    S.z[lane] = start ? fmin(fmax(wl, lo), hi) : 0.0;
  }
  if (lane == 0) S.npact = 0;
  WSYNC();
  // multipliers: y_eq, y_in uniform; y_bnd on lane j
  double y_eq0 = 0.0, y_eq1 = 0.0, y_in = 0.0, y_bnd = 0.0;
  double mu = 0.0;
  int qp_total = 0, status = PIADMM_OBCA_MAX_ITER, it = 0;
  bool have_prev = false;
  for (it = 0; it < max_iter; ++it) {
    // ---- linearise ----
    Geo G;
    geo(S.z + 9 * veh, S.z + 9 * veh + 5, prob, sigd, G);
    const double ga = ga_val(G, S.z + 9 * veh + 5);
    const double g_eq0 = __shfl(G.m[0], 0, 64) + __shfl(G.m[0], 9, 64);
    const double g_eq1 = __shfl(G.m[1], 0, 64) + __shfl(G.m[1], 9, 64);
    const double g_in = __shfl(ga, 0, 64) + __shfl(ga, 9, 64);
    for (int e = lane; e < NE * NE; e += 64) S.H0[e / NE][e % NE] = (e / NE == e % NE) ? rho : 0.0;
    WSYNC();
    if (lane == 0 || lane == 9) {
      const int b = lane;
      // gradients of this vehicle's terms
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        S.Jeq[r][b + 0] = 0.0; S.Jeq[r][b + 1] = 0.0; S.Jeq[r][b + 2] = 0.0; S.Jeq[r][b + 3] = G.mt[r]; S.Jeq[r][b + 4] = 0.0;
#pragma unroll
        for (int j = 0; j < 4; ++j) S.Jeq[r][b + 5 + j] = G.mL[r][j];
      }
      const double B0[4] = {LENGTH / 2, WIDTH / 2, LENGTH / 2, WIDTH / 2};
      S.gin[b + 0] = -G.m[0];
      S.gin[b + 1] = -G.m[1];
      S.gin[b + 2] = -dot2(G.dv, G.m);
      S.gin[b + 3] = -dot2(G.dt, G.m) - dot2(G.q, G.mt);
      S.gin[b + 4] = 0.0;
#pragma unroll
      for (int j = 0; j < 4; ++j) S.gin[b + 5 + j] = -B0[j] - (G.q[0] * G.mL[0][j] + G.q[1] * G.mL[1][j]);
      // W = rho I - y_in Hess(ga) - y_eq . Hess(m) on this vehicle's 9 x 9 block
      double (*W)[NEP] = S.H0;
      W[b + 0][b + 3] = W[b + 3][b + 0] = y_in * G.mt[0];
      W[b + 1][b + 3] = W[b + 3][b + 1] = y_in * G.mt[1];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        W[b + 0][b + 5 + j] = W[b + 5 + j][b + 0] = y_in * G.mL[0][j];
        W[b + 1][b + 5 + j] = W[b + 5 + j][b + 1] = y_in * G.mL[1][j];
        W[b + 2][b + 5 + j] = W[b + 5 + j][b + 2] = y_in * (G.dv[0] * G.mL[0][j] + G.dv[1] * G.mL[1][j]);
        W[b + 3][b + 5 + j] = W[b + 5 + j][b + 3] =
            y_in * ((G.dt[0] * G.mL[0][j] + G.dt[1] * G.mL[1][j]) + (G.q[0] * G.mtL[0][j] + G.q[1] * G.mtL[1][j]))
            - y_eq0 * G.mtL[0][j] - y_eq1 * G.mtL[1][j];
      }
      W[b + 2][b + 2] = rho + y_in * dot2(G.dvv, G.m);
      W[b + 2][b + 3] = W[b + 3][b + 2] = y_in * (dot2(G.dvt, G.m) + dot2(G.dv, G.mt));
      W[b + 3][b + 3] = rho + y_in * (dot2(G.dtt, G.m) + 2 * dot2(G.dt, G.mt) - dot2(G.q, G.m))
                        + y_eq0 * G.m[0] + y_eq1 * G.m[1];
    }
    double gfl = 0.0, zl = 0.0;
    if (lane < NE) {
      zl = S.z[lane];
      gfl = -S.lb[lane] - rho * (S.w[lane] - zl);
      S.gf[lane] = gfl;
      S.gm[lane] = gfl;
      S.din[2 + 2 * lane] = S.lo[lane] - zl;
      S.din[3 + 2 * lane] = zl - S.hi[lane];
    }
    if (lane == 0) {
      S.din[0] = min_dis - g_in;
      S.din[1] = g_in - g_max;
      S.deq[0] = -g_eq0;
      S.deq[1] = -g_eq1;
      S.sgn[0] = 1.0;
      S.sgn[1] = 1.0;
    }
    WSYNC();
    // ---- Hessian modification ----
    for (int e = lane; e < NE * NE; e += 64) S.Hm[e / NE][e % NE] = S.H0[e / NE][e % NE];
    bool pd = chol(S.Hm);
    if (!pd) {
      // Ga = sum an an' (in R), ga = sum an b / |a| over the equality rows and the previous active rows
      for (int e = lane; e < NE * NE; e += 64) S.R[e / NE][e % NE] = 0.0;
      double gal = 0.0;
      const int nprev = have_prev ? S.npact : 0;
      WSYNC();
      for (int r = 0; r < NEQ + nprev; ++r) {
        const int c = (r < NEQ) ? r : S.pact[r - NEQ];
        const double al = (lane < NE) ? ((r < NEQ) ? S.Jeq[r][lane] : row_elem(S, c, lane)) : 0.0;
        const double b = (r < NEQ) ? S.deq[r] : S.din[c];
        const double nrm = fmax(sqrt(wsum(al * al)), 1e-300);
        const double an = al / nrm;
        if (lane < NE) S.npv[lane] = an;
        WSYNC();
        if (lane < NE) {
          for (int k = 0; k < NE; ++k) S.R[lane][k] += an * S.npv[k];
          gal += an * (b / nrm);
        }
        WSYNC();
      }
      const double hmax = wmax(lane < NE ? fabs(S.H0[lane][lane]) : 0.0);
      double sig = 1e-4 * hmax;
      for (int k = 0; k < 8; ++k) {
        WSYNC();
        for (int e = lane; e < NE * NE; e += 64) S.Hm[e / NE][e % NE] = S.H0[e / NE][e % NE] + sig * S.R[e / NE][e % NE];
        if (lane < NE) S.gm[lane] = gfl - sig * gal;
        pd = chol(S.Hm);
        if (pd) break;
        if (k < 7) sig *= 10.0;
      }
      if (!pd) {
        // base = H0 + sig Ga (kept in H0), then base + tau diag(max(|base_ii|, 1e-12))
        WSYNC();
        for (int e = lane; e < NE * NE; e += 64) S.H0[e / NE][e % NE] += sig * S.R[e / NE][e % NE];
        WSYNC();
        const double dg = (lane < NE) ? fmax(fabs(S.H0[lane][lane]), 1e-12) : 0.0;
        double tau = 0.0;
        for (int k = 0; k < 16; ++k) {
          tau = (tau == 0.0) ? 1e-6 : tau * 10.0;
          WSYNC();
          for (int e = lane; e < NE * NE; e += 64) S.Hm[e / NE][e % NE] = S.H0[e / NE][e % NE];
          WSYNC();
          if (lane < NE) S.Hm[lane][lane] += tau * dg;
          pd = chol(S.Hm);
          if (pd) break;
        }
        if (!pd) { status = PIADMM_OBCA_HESSIAN_FAIL; break; }
      }
    }
    // ---- QP ----
    int qsteps = 0;
    const int qst = gi_solve(S, qsteps);
    qp_total += qsteps;
    if (qst != 0) {
      status = (qst == 2) ? PIADMM_OBCA_QP_INFEASIBLE : PIADMM_OBCA_MAX_ITER;
      break;
    }
    if (lane == 0) {
      int m = 0;
      for (int c = 0; c < NROW; ++c)
        if (S.uin[c] > 0.0) S.pact[m++] = c;
      S.npact = m;
    }
    have_prev = true;
    WSYNC();
    const double dl = (lane < NE) ? S.x[lane] : 0.0;
    const double ny_eq0 = S.ueq[0], ny_eq1 = S.ueq[1];
    const double ny_in = S.uin[0] - S.uin[1];
    const double ny_bnd = (lane < NE) ? S.uin[2 + 2 * lane] - S.uin[3 + 2 * lane] : 0.0;
    // ---- convergence ----
    const double bv = (lane < NE) ? fmax(0.0, S.lo[lane] - zl) + fmax(0.0, zl - S.hi[lane]) : 0.0;
    const double viol = fabs(g_eq0) + fabs(g_eq1) + fmax(0.0, min_dis - g_in) + fmax(0.0, g_in - g_max) + wsum(bv);
    const double step = wmax(fabs(dl));
    if (step <= TOL_STEP && viol <= TOL_FEAS) {
      if (lane < NE) S.z[lane] = zl + dl;
      y_eq0 = ny_eq0; y_eq1 = ny_eq1; y_in = ny_in; y_bnd = ny_bnd;
      status = PIADMM_OBCA_CONVERGED;
      WSYNC();
      break;
    }
    // ---- l1-merit line search ----
    const double mmax = fmax(fmax(fabs(ny_eq0), fabs(ny_eq1)), fmax(fabs(ny_in), wmax(fabs(ny_bnd))));
    mu = fmax(mu, 1.01 * mmax + 1e-6);
    const double cv = (lane < NE) ? -zl * S.lb[lane] + 0.5 * rho * (S.w[lane] - zl) * (S.w[lane] - zl) : 0.0;
    const double phi0 = wsum(cv) + mu * viol;
    const double D = wsum(gfl * dl) - mu * viol;
    double alpha = 1.0;
    bool ok = false;
    for (int k = 0; k <= MAX_HALVINGS; ++k) {
      WSYNC();
      if (lane < NE) S.zn[lane] = zl + alpha * dl;
      WSYNC();
      double ge[2], gi, vn, cn;
      point_eval(S, S.zn, prob, sigd, rho, min_dis, g_max, ge, gi, vn, cn);
      if (cn + mu * vn <= phi0 + ARMIJO * alpha * D) { ok = true; break; }
      alpha *= 0.5;
    }
    if (!ok) { status = PIADMM_OBCA_LINESEARCH_FAIL; break; }
    WSYNC();
    if (lane < NE) S.z[lane] = S.zn[lane];
    y_eq0 += alpha * (ny_eq0 - y_eq0);
    y_eq1 += alpha * (ny_eq1 - y_eq1);
    y_in += alpha * (ny_in - y_in);
    y_bnd += alpha * (ny_bnd - y_bnd);
    WSYNC();
  }
  const int iters = (it < max_iter) ? it + 1 : max_iter;
  WSYNC();
  // ---- answer, rounding, the fused lambda_update (optimizer.py:322, :330-335) ----
  double ge[2], gi, vn, cost;
  point_eval(S, S.z, prob, sigd, rho, min_dis, g_max, ge, gi, vn, cost);
  double* o = out + (size_t)pair * OUT;
  const bool wrote = status == PIADMM_OBCA_CONVERGED || status == PIADMM_OBCA_MAX_ITER ||
                     status == PIADMM_OBCA_LINESEARCH_FAIL;
  double dr = 0.0;
  if (lane < NE) {
    const int k = (veh * NT + t) * 9 + li;
    const double zf = S.z[lane], zb = around(zf, rdec);
    const double lb = S.lb[lane];
    const double lbn = wrote ? lb + rho * (S.w[lane] - zb) : lb;
    o[EO_Z + k] = zf;
    o[EO_ZB + k] = zb;
    o[EO_LBN + k] = lbn;
    o[EO_YBND + t * NE + lane] = y_bnd;
    dr = fabs(lbn - lb);
  }
  // the slot's sum |delta lamb_bar| in lane order 0..17 (bit-repeatable: no atomics)
  double dsum = 0.0;
  for (int k = 0; k < NE; ++k) dsum += __shfl(dr, k, 64);
  if (lane == 0) {
    o[EO_YEQ + 2 * t] = y_eq0;
    o[EO_YEQ + 2 * t + 1] = y_eq1;
    o[EO_YIN + t] = y_in;
    o[EO_COST + t] = cost;
    o[EO_DRES + t] = dsum;
    int* s3 = ist + ((size_t)pair * NT + t) * 3;
    s3[0] = status;
    s3[1] = iters;
    s3[2] = qp_total;
  }
}

__global__ void __launch_bounds__(64 * EW) k_obca_edge(const double* __restrict__ recs, int n_prob,
                                                       double* __restrict__ out, int* __restrict__ ist) {
  __shared__ Es S[EW];
  const int wave = threadIdx.x >> 6;
  const int pb = blockIdx.x * EW + wave;
  if (pb >= n_prob) return;          // the whole wave: waves never meet at a barrier
  edge_one(S[wave], pb / NT, pb % NT, recs, out, ist);
}

}  // namespace obca_edge

// ---------------------------------------------------------------------------------------------
// C-ABI (include/piadmm.h)
// ---------------------------------------------------------------------------------------------
namespace {
int edge_check(piadmm_obca_t h, const double* recs, int n) {
  for (int i = 0; i < n; ++i) {
    const double* par = recs + (size_t)i * obca_edge::REC + obca_edge::E_PAR;
    if (!(par[0] > 0.0) || (par[2] != 0.0 && par[2] != 1.0) || !(par[3] >= 1.0 && par[3] <= 1000.0) ||
        (par[5] != 0.0 && par[5] != 1.0) || !(par[4] >= -1.0 && par[4] <= 15.0) || !(par[6] > 0.0) || !(par[7] > 0.0) ||
        !std::isfinite(par[1]) || !std::isfinite(par[8]))
      return fail(h, PIADMM_E_ARG, "record " + std::to_string(i) + ": bad parameters (rho > 0; prob 0/1; "
                  "1 <= max_iter <= 1000; start 0/1; -1 <= round_decimals <= 15; x_bound, mu_max > 0; "
                  "min_dis, g_max finite)");
  }
  return 0;
}

int edge_ensure(piadmm_obca_t h, int n) {
  if (n <= h->e_cap) return 0;
  h->e_cap = 0;
  h->e_rec = {}; h->e_out = {}; h->e_ist = {};      // the old arrays go first (peak memory)
  int rc = 0;
  if ((rc = h->e_rec.alloc(h, (size_t)n * obca_edge::REC, false)) ||
      (rc = h->e_out.alloc(h, (size_t)n * obca_edge::OUT, false)) ||
      (rc = h->e_ist.alloc(h, (size_t)n * obca_edge::NT * 3, false)))
    return rc;
  h->e_cap = n;
  return 0;
}

int edge_upload(piadmm_obca_t h, const double* recs, int n) {
  if (!recs || n <= 0) return fail(h, PIADMM_E_ARG, "obca_edge: recs / n_pairs");
  if (int rc = edge_check(h, recs, n)) return rc;
  OWN_HIP(h, hipSetDevice(h->device));
  piadmm_obca_plan_release(h);       // the edge buffers are overwritten: an open plan ends here
  if (int rc = edge_ensure(h, n)) return rc;
  OWN_HIP(h, hipMemcpyAsync(h->e_rec, recs, (size_t)n * obca_edge::REC * sizeof(double), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemsetAsync(h->e_out, 0, (size_t)n * obca_edge::OUT * sizeof(double), h->stream));
  return 0;
}

int edge_launch(piadmm_obca_t h, int n) {
  const int n_prob = n * obca_edge::NT;
  const int blocks = (n_prob + obca_edge::EW - 1) / obca_edge::EW;
  hipLaunchKernelGGL(obca_edge::k_obca_edge, dim3(blocks), dim3(64 * obca_edge::EW), 0, h->stream, h->e_rec, n_prob,
                     h->e_out, h->e_ist);
  OWN_HIP(h, hipGetLastError());
  return 0;
}
}  // namespace

// the plan path (csrc/piadmm_obca_plan.hip): the buffers and one launch over the first n pairs
int piadmm_obca_edge_ensure(piadmm_obca_t h, int n) { return edge_ensure(h, n); }

int piadmm_obca_edge_launch(piadmm_obca_t h, int n) {
  if (n <= 0 || n > h->e_cap) return fail(h, PIADMM_E_STATE, "obca edge launch: n outside the buffers");
  return edge_launch(h, n);
}

extern "C" {

int32_t piadmm_obca_edge_solve(piadmm_obca_t h, const double* recs, int32_t n_pairs, double* out, int32_t* status3) {
  if (!h) return PIADMM_E_ARG;
  if (!out || !status3) return fail(h, PIADMM_E_ARG, "obca_edge_solve: out / status3");
  if (int rc = edge_upload(h, recs, n_pairs)) return rc;
  if (int rc = edge_launch(h, n_pairs)) return rc;
  OWN_HIP(h, hipMemcpyAsync(out, h->e_out, (size_t)n_pairs * obca_edge::OUT * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(status3, h->e_ist, (size_t)n_pairs * obca_edge::NT * 3 * sizeof(int), hipMemcpyDeviceToHost,
                         h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_edge_time(piadmm_obca_t h, const double* recs, int32_t n_pairs, int32_t repeats, float* ms) {
  if (!h || !ms || repeats <= 0) return PIADMM_E_ARG;
  if (int rc = edge_upload(h, recs, n_pairs)) return rc;
  OWN_HIP(h, hipEventRecord(h->e0, h->stream));
  for (int r = 0; r < repeats; ++r)
    if (int rc = edge_launch(h, n_pairs)) return rc;
  OWN_HIP(h, hipEventRecord(h->e1, h->stream));
  OWN_HIP(h, hipEventSynchronize(h->e1));
  float t = 0.f;
  OWN_HIP(h, hipEventElapsedTime(&t, h->e0, h->e1));
  *ms = t / (float)repeats;
  return 0;
}

}  // extern "C"
