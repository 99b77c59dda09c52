// pd_obca.h -- what the two OBCA solve kernels state once (internal, not installed): the vehicle
// constants, the record layouts, the wave reductions, the vehicle geometry, the row-owned Cholesky and
// the Goldfarb-Idnani active-set core.  csrc/piadmm_obca.hip (the local SQP: 28 variables, no
// equalities, one wave per workgroup) and csrc/piadmm_obca_edge.hip (the edge step: 18 variables, 2
// equalities, four independent waves per workgroup) instantiate the core; csrc/piadmm_obca_plan.h
// takes the constants and the layouts.  The fused MPC kernel's reductions (pd_common.h, namespace pd)
// sum in another order and are not these.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "piadmm.h"

namespace pd_obca {

constexpr int NT = 7;                          // horizon slots
// VehicleConfig (veh_config.py:7-27) and the delay statistics of OBCAOptimizer (optimizer.py:10-37)
constexpr double LENGTH = 3.5, WIDTH = 2.0;
constexpr double AVG_DELAY = 0.05, VAR_DELAY = 0.025;

// the local record and output (include/piadmm.h: PIADMM_OBCA_REC, PIADMM_OBCA_OUT doubles)
constexpr int R_INIT = 0, R_REF = 5, R_AO = 45, R_BO = 101, R_LIJ = 129, R_LB = 157, R_ZB = 220, R_PAR = 283;
constexpr int O_X = 0, O_U = 40, O_LAM = 54, O_YA = 82, O_YB = 89, O_YN = 103, O_YX = 110, O_PI = 145, O_YU = 180,
              O_YL = 194, O_COST = 222;
// the edge record and output (PIADMM_OBCA_EDGE_REC, PIADMM_OBCA_EDGE_OUT doubles)
constexpr int E_LX = 0, E_LIJ = 70, E_LB = 126, E_PAR = 252;
constexpr int EO_Z = 0, EO_ZB = 126, EO_LBN = 252, EO_YEQ = 378, EO_YIN = 392, EO_YBND = 399, EO_COST = 525,
              EO_DRES = 532;
static_assert(R_PAR + 8 <= PIADMM_OBCA_REC && O_COST + 2 == PIADMM_OBCA_OUT, "local layout");
static_assert(E_PAR + 9 <= PIADMM_OBCA_EDGE_REC && EO_DRES + NT <= PIADMM_OBCA_EDGE_OUT, "edge layout");

// ---------------------------------------------------------------------------------------------
// wave reductions (64 lanes, butterfly: every lane ends with the result)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double wsum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ double wmax(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}
// min value, lowest index on ties (idx < 0 = none)
__device__ __forceinline__ void wargmin(double& v, int& i) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    double v2 = __shfl_xor(v, o, 64);
    int i2 = __shfl_xor(i, o, 64);
    bool take = (i2 >= 0) && (i < 0 || v2 < v || (v2 == v && i2 < i));
    if (take) { v = v2; i = i2; }
  }
}

// ---------------------------------------------------------------------------------------------
// geometry of one vehicle (util.py:12-101); same closed forms as the oracle
// ---------------------------------------------------------------------------------------------
struct Geo {
  double e[2], n[2], m[2], mt[2], mL[2][4], mtL[2][4], d[2], dv[2], dvv[2], dt[2], dtt[2], dvt[2], q[2];
};

__device__ inline void geo(const double* Xt, const double* Lt, int prob, double sigd, Geo& G) {
  double v = Xt[2], th = Xt[3];
  double c = cos(th), s = sin(th);
  G.e[0] = c; G.e[1] = s; G.n[0] = -s; G.n[1] = c;
  double sg = prob ? 1.0 : -1.0;
  double a1 = Lt[0] - Lt[2], a2 = sg * (Lt[1] - Lt[3]);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    G.m[i] = a1 * G.e[i] + a2 * G.n[i];
    G.mt[i] = a1 * G.n[i] - a2 * G.e[i];
    G.mL[i][0] = G.e[i]; G.mL[i][1] = sg * G.n[i]; G.mL[i][2] = -G.e[i]; G.mL[i][3] = -sg * G.n[i];
    G.mtL[i][0] = G.n[i]; G.mtL[i][1] = -sg * G.e[i]; G.mtL[i][2] = -G.n[i]; G.mtL[i][3] = sg * G.e[i];
  }
  if (prob) {
    double k = sigd * VAR_DELAY * VAR_DELAY, da = AVG_DELAY;
    G.d[0] = da * v * c + k * v * v * c * c;           G.d[1] = da * v * s + k * v * v * s * s;
    G.dv[0] = da * c + 2 * k * v * c * c;              G.dv[1] = da * s + 2 * k * v * s * s;
    G.dvv[0] = 2 * k * c * c;                          G.dvv[1] = 2 * k * s * s;
    G.dt[0] = -da * v * s - 2 * k * v * v * c * s;     G.dt[1] = da * v * c + 2 * k * v * v * s * c;
    G.dtt[0] = -da * v * c - 2 * k * v * v * (c * c - s * s);
    G.dtt[1] = -da * v * s + 2 * k * v * v * (c * c - s * s);
    G.dvt[0] = -da * s - 4 * k * v * c * s;            G.dvt[1] = da * c + 4 * k * v * s * c;
  } else {
#pragma unroll
    for (int i = 0; i < 2; ++i) G.d[i] = G.dv[i] = G.dvv[i] = G.dt[i] = G.dtt[i] = G.dvt[i] = 0.0;
  }
  G.q[0] = Xt[0] + G.d[0];
  G.q[1] = Xt[1] + G.d[1];
}

__device__ __forceinline__ double dot2(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1]; }

// ---------------------------------------------------------------------------------------------
// The dense QP core.  A kernel describes its problem by a struct P:
//   State                 its LDS state, with Hm, J, R (N rows of stride NP), x, d, npv, dd (N), u,
//                         act (N + 1), uin (NROW), nact, and ueq, sgn (NEQ) when NEQ > 0
//   N, NP, NEQ, NROW      variables, padded row stride, equalities, inequality rows
//   lane()                the lane within the wave that owns the problem
//   fence()               what orders a write before another lane's read: the workgroup barrier
//                         where the wave is the workgroup, the wave fence where waves share one
//   elem(S, p, k)         element k of constraint p       (constraint ids: the equalities 0 .. NEQ - 1,
//   rhs(S, p)             right-hand side of constraint p  sign-normalised, then NEQ + inequality row)
// Every operation and its order inside a sum are the same for both kernels; only N differs.
// ---------------------------------------------------------------------------------------------

// Cholesky (lower, in place) of the leading n x n block of M, lane i owning row i: per column a
// pivot read, the column scaled by its owners, then each owner updates its own row (the same
// operation order per entry as the right-looking form); false if a pivot is <= thr^2 (thr = 0: not
// positive).
template <class P>
__device__ bool chol_n(double (*M)[P::NP], int n, double thr) {
  const int lane = P::lane();
  for (int j = 0; j < n; ++j) {
    P::fence();
    double piv = M[j][j];
    if (!(piv > 0.0)) { P::fence(); return false; }
    double l = sqrt(piv);
    if (!(l > thr)) { P::fence(); return false; }
    double lij = 0.0;
    if (lane > j && lane < n) { lij = M[lane][j] / l; M[lane][j] = lij; }
    if (lane == j) M[j][j] = l;
    P::fence();
    if (lane > j && lane < n)
      for (int k = j + 1; k <= lane; ++k) M[lane][k] -= lij * M[k][j];
  }
  P::fence();
  return true;
}

// Goldfarb-Idnani dual active set on min 1/2 z'Hz + g'z, equalities, C z >= din; H = L L' in S.Hm,
// J = L^-T Q, R the triangular factor of the active rows.
//
// Lane ownership inside the active-set updates: lane i owns row i of J (every Givens rotation of a
// J column pair is row-local), lane c owns column c of R during a drop's rotations; rotation
// parameters are uniform (computed by every lane from its own column and a shuffle).  So the rotation
// chain of gi_drop touches no LDS word that another lane wrote since the fence in front of it, and it
// runs without fences.  gi_drop ends with a fence and gi_add is entered behind one, so every pass of
// gi_add's loop -- the first, and each one after a drop -- starts behind a fence too: the loop has
// none at its top.  The fences that remain each order a write before another lane's read.
template <class P>
__device__ void gi_drop(typename P::State& S, int k) {
  constexpr int N = P::N;
  const int lane = P::lane();
  P::fence();
  const int q = S.nact;
  // remove column k of R (row-owned shift)
  if (lane < N) {
    for (int j = k; j < q - 1; ++j) S.R[lane][j] = S.R[lane][j + 1];
    S.R[lane][q - 1] = 0.0;
  }
  P::fence();
  for (int j = k; j < q - 1; ++j) {
    // column j is lane j's: its (R[j][j], R[j+1][j]) after the previous rotations
    double aj = (lane < N) ? S.R[j][lane] : 0.0;
    double bj = (lane < N) ? S.R[j + 1][lane] : 0.0;
    double a = __shfl(aj, j, 64), b = __shfl(bj, j, 64);
    double h = hypot(a, b);
    if (h != 0.0) {
      double cs = a / h, sn = b / h;
      if (lane >= j && lane < q - 1) {
        S.R[j][lane] = cs * aj + sn * bj;
        S.R[j + 1][lane] = -sn * aj + cs * bj;
      }
      if (lane < N) {
        double Jj = S.J[lane][j], Jj1 = S.J[lane][j + 1];
        S.J[lane][j] = cs * Jj + sn * Jj1;
        S.J[lane][j + 1] = -sn * Jj + cs * Jj1;
      }
    }
  }
  P::fence();
  if (lane == 0) {
    for (int j = k; j < q - 1; ++j) { S.act[j] = S.act[j + 1]; S.u[j] = S.u[j + 1]; }
    S.nact = q - 1;
  }
  P::fence();
}

// constraint p joins the active set; returns 1 added, 0 infeasible, -1 step limit
template <class P>
__device__ int gi_add(typename P::State& S, int p, int& steps) {
  constexpr int N = P::N;
  const int lane = P::lane();
  double up = 0.0;
  const double bp = P::rhs(S, p);
  P::fence();
  if (lane < N) S.npv[lane] = P::elem(S, p, lane);
  P::fence();
  const double npl = (lane < N) ? S.npv[lane] : 0.0;
  while (true) {
    if (++steps > 500) return -1;
    const int q = S.nact;
    // d = J' n_p (lane j)
    double dj = 0.0;
    if (lane < N)
      for (int i = 0; i < N; ++i) dj += S.J[i][lane] * S.npv[i];
    if (lane < N) S.d[lane] = dj;
    P::fence();
    // z = J[:, q:] d[q:] (lane i)
    double zi = 0.0;
    if (lane < N)
      for (int j = q; j < N; ++j) zi += S.J[lane][j] * S.d[j];
    // r = R^-1 d[:q]: back substitution on the lanes' registers (lane k ends with r_k)
    double ddk = (lane < q) ? dj : 0.0, rk = 0.0;
    for (int j = q - 1; j >= 0; --j) {
      double rj = __shfl(ddk, j, 64) / S.R[j][j];
      if (lane == j) rk = rj;
      if (lane < j) ddk -= S.R[lane][j] * rj;
    }
    // partial step t1 over the active inequalities with r_k > 1e-13 max(1, max|r|)
    const double rmax = fmax(1.0, wmax(lane < q ? fabs(rk) : 0.0));
    double t1v = INFINITY;
    int l = -1;
    bool leaves = lane < q;
    if constexpr (P::NEQ > 0) leaves = leaves && S.act[lane] >= P::NEQ;      // an equality never leaves
    if (leaves && rk > 1e-13 * rmax) { t1v = S.u[lane] / rk; l = lane; }
    wargmin(t1v, l);
    const double t1 = (l >= 0) ? t1v : INFINITY;
    // full step t2
    const double xl = (lane < N) ? S.x[lane] : 0.0;
    const double zn = wsum(zi * npl);
    const double dd2 = wsum(dj * dj);
    const double sx = wsum(npl * xl) - bp;
    const double t2 = (zn > 1e-12 * dd2) ? -sx / zn : INFINITY;
    const double t = fmin(t1, t2);
    if (t == INFINITY) return 0;
    if (t2 == INFINITY) {
      if (lane < q) S.u[lane] -= t * rk;
      up += t;
      gi_drop<P>(S, l);
      continue;
    }
    if (lane < N) S.x[lane] = xl + t * zi;
    if (lane < q) S.u[lane] -= t * rk;
    up += t;
    if (t == t2) {
      // one Householder reflection of J[:, q:] zeroing d[q+1..] (uniform v, each lane its own row)
      double alpha = S.d[q];
      if (q < N - 1) {
        double ss = 0.0;
        for (int j = q + 1; j < N; ++j) ss += S.d[j] * S.d[j];
        if (ss > 0.0) {
          const double a0 = S.d[q];
          const double sig = sqrt(a0 * a0 + ss);
          alpha = (a0 > 0.0) ? -sig : sig;
          const double v0 = a0 - alpha;
          const double beta = 1.0 / (sig * (sig + fabs(a0)));     // 2 / v'v
          if (lane < N) {
            double sv = S.J[lane][q] * v0;
            for (int j = q + 1; j < N; ++j) sv += S.J[lane][j] * S.d[j];
            sv *= beta;
            S.J[lane][q] -= sv * v0;
            for (int j = q + 1; j < N; ++j) S.J[lane][j] -= sv * S.d[j];
          }
        }
      }
      if (lane < q) S.R[lane][q] = S.d[lane];
      if (lane == q) S.R[q][q] = alpha;
      P::fence();
      if (lane == 0) { S.act[q] = p; S.u[q] = up; S.nact = q + 1; }
      P::fence();
      return 1;
    }
    gi_drop<P>(S, l);
  }
}

// The opening of a solve: J = L^-T (row j of J is column j of L^-1, forward substitution of
// L y = e_j, lane j its row) and S.dd = J' g.
template <class P>
__device__ __forceinline__ void gi_factor(typename P::State& S, const double* g) {
  constexpr int N = P::N;
  const int lane = P::lane();
  if (lane < N) {
    const int j = lane;
    double* y = S.J[j];
    for (int i = 0; i < N; ++i) {
      if (i < j) { y[i] = 0.0; continue; }
      double s = (i == j) ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) s -= S.Hm[i][k] * y[k];
      y[i] = s / S.Hm[i][i];
    }
  }
  P::fence();
  if (lane < N) {
    double s = 0.0;
    for (int i = 0; i < N; ++i) s += S.J[i][lane] * g[i];
    S.dd[lane] = s;
  }
  P::fence();
}
// ... then the unconstrained minimiser x = -J J' g and the empty active set
template <class P>
__device__ __forceinline__ void gi_start(typename P::State& S) {
  constexpr int N = P::N;
  const int lane = P::lane();
  if (lane < N) {
    double s = 0.0;
    for (int j = 0; j < N; ++j) s += S.J[lane][j] * S.dd[j];
    S.x[lane] = -s;
  }
  for (int e = lane; e < N * N; e += 64) S.R[e / N][e % N] = 0.0;
  if (lane == 0) S.nact = 0;
  P::fence();
}
// The closing: the active set's u scattered into the dense multipliers S.uin (and S.ueq, the
// equalities' sign normalisation undone).
template <class P>
__device__ __forceinline__ void gi_multipliers(typename P::State& S) {
  const int lane = P::lane();
  P::fence();
  for (int c = lane; c < P::NROW; c += 64) S.uin[c] = 0.0;
  if constexpr (P::NEQ > 0)
    if (lane < P::NEQ) S.ueq[lane] = 0.0;
  P::fence();
  if (lane == 0)
    for (int k = 0; k < S.nact; ++k) {
      const double uk = S.u[k];
      const int c = S.act[k];
      if constexpr (P::NEQ > 0)
        if (c < P::NEQ) { S.ueq[c] = uk * S.sgn[c]; continue; }
      S.uin[c - P::NEQ] = uk;
    }
  P::fence();
}

}  // namespace pd_obca
