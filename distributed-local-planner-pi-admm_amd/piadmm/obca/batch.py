"""The batch handle: every launch on the call's own buffers (piadmm_obca_*, include/piadmm.h)."""
import ctypes

import numpy as np

from .. import _lib
from .._lib import DELAY_PAR, DUAL_PAR, FEEDBACK_PAR, NOISE_PAR
from .feedback import _draw_rows
from .model import (_EO_COST, _EO_DRES, _EO_LBN, _EO_YBND, _EO_YEQ, _EO_YIN, _EO_Z, _EO_ZB, EDGE_OUT, EDGE_REC, N_HORZ,
                    NE, NT, NU, NX, OUT, REC)
from .stats import OBCAFleetStats, _stats_call


class OBCAEdgeResult:
    """Decoded output of an edge batch (pairs x ...)."""

    def __init__(self, out, ist):
        n = out.shape[0]
        self.raw = out
        self.Z = out[:, _EO_Z:_EO_Z + 126].reshape(n, 2, NT, 9)
        self.Z_bar = out[:, _EO_ZB:_EO_ZB + 126].reshape(n, 2, NT, 9)
        self.lamb_bar = out[:, _EO_LBN:_EO_LBN + 126].reshape(n, 2, NT, 9)
        self.y_eq = out[:, _EO_YEQ:_EO_YEQ + 14].reshape(n, NT, 2)
        self.y_in = out[:, _EO_YIN:_EO_YIN + 7]
        self.y_bnd = out[:, _EO_YBND:_EO_YBND + 126].reshape(n, NT, NE)
        self.cost = out[:, _EO_COST:_EO_COST + 7]
        self.dres = out[:, _EO_DRES:_EO_DRES + 7]
        self.status = ist[:, :, 0]
        self.iters = ist[:, :, 1]
        self.qp_steps = ist[:, :, 2]

    def z(self, k, t):
        """The 18 variables [s_0, mu_0, s_1, mu_1] of pair k, slot t."""
        return np.concatenate([self.Z[k, 0, t], self.Z[k, 1, t]])

    def dual_residual(self):
        """sum |lamb_bar_new - lamb_bar| per pair: the 7 slot partials added in index order."""
        s = np.zeros(self.dres.shape[0])
        for t in range(NT):
            s = s + self.dres[:, t]
        return s


class OBCAResult:
    """Decoded output of a batch (fields as in the reference's local_solve, :183-201)."""

    def __init__(self, out, ist):
        self.raw = out
        self.X = out[:, :40].reshape(-1, 8, 5)
        self.U = out[:, 40:54].reshape(-1, 7, 2)
        self.Lam = out[:, 54:82].reshape(-1, 7, 4)
        self.y_a = out[:, 82:89]
        self.y_b = out[:, 89:103].reshape(-1, 7, 2)
        self.y_n = out[:, 103:110]
        self.y_x = out[:, 110:145].reshape(-1, 7, 5)
        self.pi = out[:, 145:180].reshape(-1, 7, 5)
        self.y_u = out[:, 180:194]
        self.y_l = out[:, 194:222]
        self.cost = out[:, 222]
        self.status = ist[:, 0]
        self.iters = ist[:, 1]
        self.qp_steps = ist[:, 2]

    def bar_fullx(self, k):
        """N_horz-1 x 9 [X_t, Lambda_t] of problem k (optimizer.py:201)."""
        return np.concatenate([self.X[k, 1:], self.Lam[k]], axis=1)


class OBCABatch:
    """Device-resident batch of local problems.  ``solve`` runs one launch of the batched SQP
    (one wave per problem) and returns an OBCAResult; there is no CPU path."""

    def __init__(self, device: int = 0):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        rc = self._lib.piadmm_obca_create(int(device), ctypes.byref(self._h))
        if rc != 0:
            raise _lib.PiadmmError(f"piadmm_obca_create failed ({rc})")

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.piadmm_obca_last_error(self._h)
            raise _lib.PiadmmError(f"libpiadmm error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if self._h:
            self._lib.piadmm_obca_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, recs: np.ndarray) -> OBCAResult:
        recs = np.ascontiguousarray(recs, np.float64)
        n = recs.shape[0]
        assert recs.shape == (n, REC)
        out = np.zeros((n, OUT))
        ist = np.zeros((n, 3), np.int32)
        self._check(self._lib.piadmm_obca_solve(self._h, _lib.dptr(recs), n, _lib.dptr(out), _lib.iptr(ist)))
        return OBCAResult(out, ist)

    def solve_edge(self, recs: np.ndarray) -> OBCAEdgeResult:
        """One launch of the edge SQP (one wave per slot problem, 7 per pair) with the fused
        lambda_update; separate device buffers from the local batch."""
        recs = np.ascontiguousarray(recs, np.float64)
        n = recs.shape[0]
        assert recs.shape == (n, EDGE_REC)
        out = np.zeros((n, EDGE_OUT))
        ist = np.zeros((n, NT, 3), np.int32)
        self._check(self._lib.piadmm_obca_edge_solve(self._h, _lib.dptr(recs), n, _lib.dptr(out), _lib.iptr(ist)))
        return OBCAEdgeResult(out, ist)

    def clearance(self, states, prob) -> np.ndarray:
        """n x 2 (plain, tight) clearances of the state pairs `states` (n x 2 x 5), one launch of
        k_plan_clearance on the call's own buffers; prob: one value or one per pair."""
        states = np.ascontiguousarray(states, np.float64)
        n = states.shape[0] if states.ndim == 3 else 0
        assert states.shape == (n, 2, NX), states.shape
        prob = np.ascontiguousarray(np.broadcast_to(np.asarray(prob, np.int32), (n,)))
        out = np.zeros((n, 2))
        self._check(self._lib.piadmm_obca_clearance(self._h, n, _lib.dptr(states), _lib.iptr(prob), _lib.dptr(out)))
        return out

    def dual_pi(self, w, zb, lamb, status, gains, S, D):
        """One launch of k_plan_dual_pi on the call's own buffers (piadmm_obca_dual_pi): w, zb, lamb,
        S, D n x 2 x 7 x 9, status n x 7, gains one row or n rows of DUAL_PAR.  Returns
        (lamb_out, S', D', dres n x 7); the arguments stay as they are."""
        w = np.ascontiguousarray(w, np.float64)
        n = w.shape[0] if w.ndim == 4 else 0
        shp = (n, 2, NT, 9)
        zb, lamb = np.ascontiguousarray(zb, np.float64), np.ascontiguousarray(lamb, np.float64)
        S, D = np.array(S, np.float64, order="C"), np.array(D, np.float64, order="C")
        assert w.shape == zb.shape == lamb.shape == S.shape == D.shape == shp, (w.shape, zb.shape, S.shape)
        status = np.ascontiguousarray(status, np.int32)
        assert status.shape == (n, NT), status.shape
        gains = np.ascontiguousarray(np.atleast_2d(np.asarray(gains, np.float64)))
        assert gains.ndim == 2 and gains.shape[1] == DUAL_PAR, gains.shape
        lamb_out, dres = np.zeros(shp), np.zeros((n, NT))
        self._check(self._lib.piadmm_obca_dual_pi(self._h, n, _lib.dptr(w), _lib.dptr(zb), _lib.dptr(lamb),
                                                  _lib.iptr(status), _lib.dptr(gains), gains.shape[0], _lib.dptr(S),
                                                  _lib.dptr(D), _lib.dptr(lamb_out), _lib.dptr(dres)))
        return lamb_out, S, D, dres

    def order(self, lst, work) -> np.ndarray:
        """One launch of k_plan_order on the call's own buffers (piadmm_obca_order): the m distinct
        scenarios of `lst` sorted by `work` (n x 2), as `plan_order` states it."""
        lst = np.ascontiguousarray(lst, np.int32).reshape(-1)
        work = np.ascontiguousarray(work, np.int32)
        assert work.ndim == 2 and work.shape[1] == 2, work.shape
        out = np.zeros(len(lst), np.int32)
        self._check(self._lib.piadmm_obca_order(self._h, _lib.iptr(lst), len(lst), _lib.iptr(work), work.shape[0],
                                                _lib.iptr(out)))
        return out

    def clock_tick(self, clock, ran, ref):
        """One launch each of k_plan_clock and k_plan_compact on the call's own buffers
        (piadmm_obca_clock_tick): clock n x 3, ran n, ref 2 x n_ref x 5 or n x 2 x n_ref x 5.
        Returns (clock_out, window n x 2 x 8 x 5, the alive scenarios ascending), as `clock_tick` /
        `clock_window` state them."""
        clock = np.ascontiguousarray(clock, np.int32)
        n = clock.shape[0]
        assert clock.shape == (n, 3), clock.shape
        ran = np.ascontiguousarray(ran, np.int32)
        ref = np.ascontiguousarray(ref, np.float64)
        assert ran.shape == (n,) and ref.shape[-3] == 2 and ref.shape[-1] == NX, (ran.shape, ref.shape)
        rows = ref.shape[0] if ref.ndim == 4 else 1
        out, win = np.zeros((n, 3), np.int32), np.zeros((n, 2, N_HORZ, NX))
        lst, count = np.zeros(n, np.int32), np.zeros(1, np.int32)
        self._check(self._lib.piadmm_obca_clock_tick(self._h, n, _lib.iptr(clock), _lib.iptr(ran), _lib.dptr(ref), rows,
                                                     ref.shape[-2], _lib.iptr(out), _lib.dptr(win), _lib.iptr(lst),
                                                     _lib.iptr(count)))
        assert 0 <= count[0] <= n and not lst[count[0]:].any()
        return out, win, lst[:count[0]].copy()

    def propagate(self, states, ctrl, par, w=None) -> np.ndarray:
        """One launch of k_plan_propagate on the call's own buffers (piadmm_obca_propagate): the
        states n x 2 x 5 the vehicles reach from `states` under the held controls ctrl (n x 2 x 2:
        a, omega), the plant rows par (one for all, or n) and the disturbance w (n x 2 x 5 or None),
        as `propagate` states it."""
        states = np.ascontiguousarray(states, np.float64)
        n = states.shape[0] if states.ndim == 3 else 0
        ctrl = np.ascontiguousarray(ctrl, np.float64)
        assert states.shape == (n, 2, NX) and ctrl.shape == (n, 2, NU), (states.shape, ctrl.shape)
        par = np.ascontiguousarray(np.broadcast_to(np.asarray(par, np.float64).reshape(-1, FEEDBACK_PAR),
                                                   (n, FEEDBACK_PAR)))
        if w is not None:
            w = np.ascontiguousarray(w, np.float64)
            assert w.shape == states.shape, w.shape
        out = np.zeros((n, 2, NX))
        self._check(self._lib.piadmm_obca_propagate(self._h, n, _lib.dptr(states), _lib.dptr(ctrl), _lib.dptr(par),
                                                    _lib.dptr(w), _lib.dptr(out)))
        return out

    def noise_tape(self, n, cap, par, streams=None, seed=0, k0=0, raw=False):
        """k_plan_noise on the call's own buffers (piadmm_obca_noise_tape): the disturbance rows
        n x cap x 2 x 5 of the streams `streams` (None: 0 .. n-1) at step indices k0 .. k0 + cap - 1
        under the noise rows par (one for all, or n), as `noise_tape` states them; with raw=True
        also the generator's words, n x cap x 2 x 3 x 4 uint32 (`noise_raw`).  The library checks
        the arguments."""
        n, cap = int(n), int(cap)
        par, streams = _draw_rows(par, NOISE_PAR, streams, n)
        tape = np.zeros((max(n, 0), max(cap, 0), 2, NX))
        words = np.zeros((max(n, 0), max(cap, 0), 2, 3, 4), np.uint32) if raw else None
        self._check(self._lib.piadmm_obca_noise_tape(
            self._h, n, cap, _lib.dptr(par), par.shape[0], _lib.i64ptr(streams), ctypes.c_uint64(int(seed)), int(k0),
            _lib.dptr(tape), _lib.u32ptr(words)))
        return (tape, words) if raw else tape

    def delay_tau(self, n, cap, par, streams=None, seed=0, k0=0, tape=None, raw=False):
        """k_plan_delay on the call's own buffers (piadmm_obca_delay_tau): the latencies n x cap x 2
        of the streams `streams` (None: 0 .. n-1) at step indices k0 .. k0 + cap - 1 under the delay
        rows par (one for all, or n) and the recorded latencies tape (n x cap x 2 or None), as
        `delay_tau` states them; with raw=True also the call's words, n x cap x 2 x 4 uint32
        (`noise_raw` with calls=(3,)).  The library checks the arguments."""
        n, cap = int(n), int(cap)
        par, streams = _draw_rows(par, DELAY_PAR, streams, n)
        if tape is not None:
            tape = np.ascontiguousarray(tape, np.float64)
            assert tape.shape == (n, cap, 2), tape.shape
        tau = np.zeros((max(n, 0), max(cap, 0), 2))
        words = np.zeros((max(n, 0), max(cap, 0), 2, 4), np.uint32) if raw else None
        self._check(self._lib.piadmm_obca_delay_tau(
            self._h, n, cap, _lib.dptr(par), par.shape[0], _lib.i64ptr(streams), ctypes.c_uint64(int(seed)), int(k0),
            _lib.dptr(tape), _lib.dptr(tau), _lib.u32ptr(words)))
        return (tau, words) if raw else tau

    def loop_draw(self, clock, noise=None, delay=None, streams=None, seed=0, k0=0):
        """k_loop_draw on the call's own buffers (piadmm_obca_loop_draw): (w n x 2 x 5, tau n x 2), the
        disturbance row and the latency of stream streams[s] (None: s) at step index k0 + clock[s][0]
        under the noise / delay rows (one for all, or n; None: zeros), as `loop_draw` states them.
        clock n x 3 as the CLOCK item.  The library checks the arguments."""
        clock = np.ascontiguousarray(clock, np.int32)
        n = clock.shape[0]
        assert clock.shape == (n, 3), clock.shape
        noise = None if noise is None else _draw_rows(noise, NOISE_PAR, None, n)[0]
        delay = None if delay is None else _draw_rows(delay, DELAY_PAR, None, n)[0]
        if streams is not None:
            streams = np.ascontiguousarray(streams, np.int64).reshape(-1)
            assert streams.shape == (n,), streams.shape
        w, tau = np.zeros((n, 2, NX)), np.zeros((n, 2))
        self._check(self._lib.piadmm_obca_loop_draw(
            self._h, n, _lib.iptr(clock), _lib.dptr(noise), 0 if noise is None else noise.shape[0], _lib.dptr(delay),
            0 if delay is None else delay.shape[0], _lib.i64ptr(streams), ctypes.c_uint64(int(seed)), int(k0),
            _lib.dptr(w), _lib.dptr(tau)))
        return w, tau

    def delay_exchange(self, X, prob, tau):
        """The stale message alone, one launch of k_delay_exchange on the call's own buffers
        (piadmm_obca_delay_exchange): X n x 2 x 8 x 5 the local solves' states, prob one value or one
        per scenario, tau n x 2 latencies in [0, DT].  Returns (local_x n x 2 x 7 x 5, A n x 2 x 7 x
        4 x 2, b n x 2 x 7 x 4): `stale_states` and `halfspaces` of it."""
        X = np.ascontiguousarray(X, np.float64)
        n = X.shape[0] if X.ndim == 4 else 0
        tau = np.ascontiguousarray(tau, np.float64)
        assert X.shape == (n, 2, N_HORZ, NX) and tau.shape == (n, 2), (X.shape, tau.shape)
        prob = np.ascontiguousarray(np.broadcast_to(np.asarray(prob, np.int32), (n,)))
        lx, A, b = np.zeros((n, 2, NT, NX)), np.zeros((n, 2, NT, 4, 2)), np.zeros((n, 2, NT, 4))
        self._check(self._lib.piadmm_obca_delay_exchange(self._h, n, _lib.dptr(X), _lib.iptr(prob), _lib.dptr(tau),
                                                         _lib.dptr(lx), _lib.dptr(A), _lib.dptr(b)))
        return lx, A, b

    def fleet_stats(self, clear, summary, iters=None, mask=None, edges=(0.0,), worst=1) -> OBCAFleetStats:
        """The fleet statistics of the caller's arrays (piadmm_obca_fleet_stats: k_stats_fleet,
        k_stats_rows and k_stats_worst on the call's own buffers), as `fleet_stats_host` states them:
        clear (R + 1) x n x 2, summary n x 4, iters R x n and mask R x n x 2 (None for R = 0)."""
        clear, summary = np.ascontiguousarray(clear, np.float64), np.ascontiguousarray(summary, np.float64)
        R, n = clear.shape[0] - 1, clear.shape[1]
        assert clear.shape == (R + 1, n, 2) and summary.shape == (n, 4), (clear.shape, summary.shape)
        iters = None if iters is None else np.ascontiguousarray(iters, np.int32)
        mask = None if mask is None else np.ascontiguousarray(mask, np.int32)
        assert iters is None or iters.shape == (R, n), iters.shape
        assert mask is None or mask.shape == (R, n, 2), mask.shape

        def call(*a):
            return self._lib.piadmm_obca_fleet_stats(self._h, R, n, _lib.dptr(clear), _lib.dptr(summary),
                                                     _lib.iptr(iters) if R else None, _lib.iptr(mask) if R else None, *a)
        rc, out = _stats_call(call, n, R, edges, worst)
        self._check(rc)
        return out

    def time_edge(self, recs: np.ndarray, repeats: int) -> float:
        """ms per edge launch over `repeats` launches of `recs` (HIP events)."""
        recs = np.ascontiguousarray(recs, np.float64)
        ms = ctypes.c_float()
        self._check(self._lib.piadmm_obca_edge_time(self._h, _lib.dptr(recs), recs.shape[0], int(repeats),
                                                    ctypes.byref(ms)))
        return ms.value

    def upload(self, recs: np.ndarray):
        recs = np.ascontiguousarray(recs, np.float64)
        self._check(self._lib.piadmm_obca_upload(self._h, _lib.dptr(recs), recs.shape[0]))

    def run_async(self, repeats: int = 1):
        self._check(self._lib.piadmm_obca_run(self._h, int(repeats)))

    def time(self, repeats: int) -> float:
        """ms per launch over `repeats` launches on the resident batch (HIP events)."""
        ms = ctypes.c_float()
        self._check(self._lib.piadmm_obca_time(self._h, int(repeats), ctypes.byref(ms)))
        return ms.value

    def download(self, n: int) -> OBCAResult:
        out = np.zeros((n, OUT))
        ist = np.zeros((n, 3), np.int32)
        self._check(self._lib.piadmm_obca_download(self._h, _lib.dptr(out), _lib.iptr(ist), n))
        return OBCAResult(out, ist)
