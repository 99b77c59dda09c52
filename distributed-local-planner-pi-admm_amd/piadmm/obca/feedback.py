"""Closing the loop (csrc/piadmm_obca_plan_feedback.hip, piadmm_obca_plan_delay.hip), in NumPy: the plant, the
Philox generator, and the disturbance noise and the communication delay drawn from it."""
import math

import numpy as np

from .._lib import DELAY_PAR, FEEDBACK_PAR, NOISE_PAR
from .model import DT, NU, NX


# a plant row of the closed-loop feedback (piadmm_obca_feedback_plan / piadmm_obca_propagate,
# include/piadmm.h): these 8 doubles per vehicle, vehicle 0 first, FEEDBACK_PAR doubles in all
FEEDBACK_ROW = ("method", "n_sub", "lr", "lf", "gain_a", "gain_w", "a_max", "w_max")
FEEDBACK_N_SUB_MAX = 64
MAX_STEER = 0.6                       # max_front_wheel_angle (veh_config.py)
# the nominal plant: the NLP's own transition st + dt f(st, con) (optimizer.py:92-96)
_FEEDBACK_DEFAULT = dict(method=0, n_sub=1, lr=1.0, lf=1.5, gain_a=1.0, gain_w=1.0, a_max=5.0, w_max=20.0)


def feedback_row(**kw):
    """One plant row (FEEDBACK_PAR doubles) from FEEDBACK_ROW names, each one value for both vehicles
    or a pair (vehicle 0, vehicle 1); absent: the nominal plant (Euler, n_sub 1, lr 1.0, lf 1.5,
    gains 1, a_max 5, w_max 20)."""
    assert set(kw) <= set(FEEDBACK_ROW), set(kw) - set(FEEDBACK_ROW)
    row = np.zeros((2, len(FEEDBACK_ROW)))
    for j, k in enumerate(FEEDBACK_ROW):
        row[:, j] = np.broadcast_to(np.asarray(kw.get(k, _FEEDBACK_DEFAULT[k]), np.float64), (2,))
    return row.reshape(FEEDBACK_PAR)


def feedback_row_check(row):
    """None when the plant row is good, else what is wrong with it: the library's check."""
    row = np.asarray(row, np.float64).reshape(2, len(FEEDBACK_ROW))
    if not np.isfinite(row).all():
        return "every entry finite"
    for method, n_sub, lr, lf, _, _, a_max, w_max in row:
        if method not in (0.0, 1.0):
            return "method 0 (Euler) or 1 (RK4)"
        if not (1.0 <= n_sub <= FEEDBACK_N_SUB_MAX and n_sub == math.floor(n_sub)):
            return "1 <= n_sub <= 64, an integer"
        if not (lr > 0.0 and lf > 0.0):
            return "lr, lf > 0"
        if not (a_max > 0.0 and w_max > 0.0):
            return "a_max, w_max > 0"
    return None


def _plant_rhs(x, a_eff, w_eff, lr, lf):
    """The reference's right-hand side (optimizer.py:75-77) of the states x (..., 5)."""
    beta = np.arctan(lr * np.tan(x[..., 4]) / (lr + lf))
    ph = x[..., 3] + beta
    v = x[..., 2]
    return np.stack((v * np.cos(ph), v * np.sin(ph), a_eff, v / lr * np.sin(beta), w_eff), axis=-1)


def propagate(states, ctrl, par, w=None):
    """One plant step of length DT per vehicle, host restatement of k_plan_propagate
    (csrc/piadmm_obca_plan_feedback.hip) with the same statements in the same order: states n x 2 x 5
    (x, y, v, theta, delta), ctrl n x 2 x 2 the held (a, omega), par one plant row for all or n rows
    (`feedback_row`), w n x 2 x 5 the disturbance or None.  n_sub substeps of DT / n_sub of
        beta = atan(lr tan(delta) / (lr + lf))
        rhs = (v cos(theta + beta), v sin(theta + beta), a_eff, v / lr sin(beta), w_eff)
    with a_eff = clip(gain_a a, +-a_max), w_eff = clip(gain_w omega, +-w_max): explicit Euler
    (method 0) or classical RK4 (method 1), delta clipped to +-MAX_STEER after every substep, w added
    after the last.  The nominal row with w = None is st + DT f(st, con)."""
    x = np.array(states, np.float64)
    n = x.shape[0] if x.ndim == 3 else 0
    ctrl = np.asarray(ctrl, np.float64)
    assert x.shape == (n, 2, NX) and ctrl.shape == (n, 2, NU), (x.shape, ctrl.shape)
    P = np.broadcast_to(np.asarray(par, np.float64).reshape(-1, 2, len(FEEDBACK_ROW)), (n, 2, len(FEEDBACK_ROW)))
    for k in range(n):
        why = feedback_row_check(P[k])
        if why is not None:
            raise ValueError(f"obca.propagate: row {k}: {why}")
    rk4, n_sub, lr, lf = P[..., 0] != 0.0, P[..., 1].astype(np.int64), P[..., 2], P[..., 3]
    a_eff = np.minimum(P[..., 6], np.maximum(P[..., 4] * ctrl[..., 0], -P[..., 6]))
    w_eff = np.minimum(P[..., 7], np.maximum(P[..., 5] * ctrl[..., 1], -P[..., 7]))
    hs = (DT / n_sub.astype(np.float64))[..., None]
    for sub in range(int(n_sub.max()) if n else 0):
        k1 = _plant_rhs(x, a_eff, w_eff, lr, lf)
        nxt = x + hs * k1
        if rk4.any():
            k2 = _plant_rhs(x + (0.5 * hs) * k1, a_eff, w_eff, lr, lf)
            k3 = _plant_rhs(x + (0.5 * hs) * k2, a_eff, w_eff, lr, lf)
            k4 = _plant_rhs(x + hs * k3, a_eff, w_eff, lr, lf)
            acc = k1 + 2.0 * k2 + 2.0 * k3 + k4
            nxt = np.where(rk4[..., None], x + (hs / 6.0) * acc, nxt)
        nxt[..., 4] = np.minimum(MAX_STEER, np.maximum(nxt[..., 4], -MAX_STEER))
        x = np.where((sub < n_sub)[..., None], nxt, x)
    if w is not None:
        w = np.asarray(w, np.float64)
        assert w.shape == x.shape, (w.shape, x.shape)
        x = x + w
    return x


def feedback_args(n, feedback):
    """(par, tape) of a planner's feedback argument dict(par=, tape=): par one plant row or n rows
    (None: the nominal row), as rows x FEEDBACK_PAR; tape n x cap x 2 x 5 or None."""
    assert set(feedback) <= {"par", "tape"}, set(feedback)
    par, tape = feedback.get("par"), feedback.get("tape")
    par = feedback_row() if par is None else par
    par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, FEEDBACK_PAR))
    assert par.shape[0] in (1, n), par.shape
    if tape is not None:
        tape = np.ascontiguousarray(tape, np.float64)
        assert tape.ndim == 4 and tape.shape[0] == n and tape.shape[2:] == (2, NX), tape.shape
    return par, tape


# the device-side disturbance noise (piadmm_obca_noise_plan / piadmm_obca_noise_tape,
# include/piadmm.h): a noise row (NOISE_PAR doubles) is sigma[2][5], bias[2][5], trunc and one reserved zero
NOISE_K_MAX = 1 << 31                 # step indices stay below it
# the noise items of piadmm_obca_plan_get: name -> (code, dtype) (PIADMM_OBCA_NOISE_GET_*)
NOISE_GET = {"NOISE_PAR": (36, np.float64), "NOISE_STREAMS": (37, np.int64), "NOISE_SEED": (38, np.uint64)}
_PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
_PHILOX_W = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), vectorised over leading axes: counter
    (..., 4) and key (..., 2) 32-bit words (broadcast against each other), the result (..., 4)
    uint32.  Ten rounds; a round takes the 64-bit products of the multipliers 0xD2511F53 with c0 and
    0xCD9E8D57 with c2 to (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), the key bumped by 0x9E3779B9 and
    0xBB67AE85 between rounds.  k_plan_noise runs the same statements in 32-bit registers."""
    c = np.asarray(counter).astype(np.uint64) & _U32
    k = np.asarray(key).astype(np.uint64) & _U32
    assert c.shape[-1] == 4 and k.shape[-1] == 2, (c.shape, k.shape)
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead) for i in range(2))
    for _ in range(10):
        p0, p1 = _PHILOX_M[0] * c0, _PHILOX_M[1] * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _PHILOX_W[0]) & _U32, (k1 + _PHILOX_W[1]) & _U32
    return np.stack((c0, c1, c2, c3), axis=-1).astype(np.uint32)


def noise_raw(seed, streams, k, calls=(0, 1, 2)):
    """The generator's words of the streams `streams` (m int64, >= 0) at step index k: m x 2 x 3 x 4
    uint32, the call j of vehicle v at counter (k, 4 v + j, t & 0xffffffff, t >> 32) under the key
    (seed & 0xffffffff, seed >> 32).  calls: the call indices j (each below 4), the third axis; the
    noise's are 0, 1, 2 and the communication delay's is 3 (`delay_tau`)."""
    t = np.asarray(streams, np.int64).reshape(-1)
    seed, k = int(seed), int(k)
    calls = np.asarray(calls, np.int64).reshape(-1)
    assert (t >= 0).all() and 0 <= seed < 1 << 64 and 0 <= k < NOISE_K_MAX, (seed, k)
    assert ((calls >= 0) & (calls < 4)).all(), calls
    t = t.astype(np.uint64)
    counter = np.zeros((len(t), 2, len(calls), 4), np.uint64)
    counter[..., 0] = k
    counter[..., 1] = (4 * np.arange(2)[:, None] + calls[None, :])[None]
    counter[..., 2] = (t & _U32)[:, None, None]
    counter[..., 3] = (t >> np.uint64(32))[:, None, None]
    return philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def noise_uniform(seed, streams, k, calls=(0, 1, 2)):
    """The uniforms of `noise_raw`: m x 2 x 3 x 2 fp64, (u1, u2) of every call,
    u = (((hi << 32 | lo) >> 12) + 0.5) 2^-52 -- 52 bits and the half, exact in fp64 and strictly
    inside (0, 1)."""
    r = noise_raw(seed, streams, k, calls).astype(np.uint64)
    a = (r[..., 0::2] << np.uint64(32) | r[..., 1::2]) >> np.uint64(12)
    return (a.astype(np.float64) + 0.5) * 2.0 ** -52


def _box_muller(u):
    """(rad cos(ang), rad sin(ang)) with rad = sqrt(-2 log(u1)) and ang = 2 pi u2 of u = (..., 2) uniforms."""
    rad = np.sqrt(-2.0 * np.log(u[..., 0]))
    ang = (2.0 * np.pi) * u[..., 1]
    return rad * np.cos(ang), rad * np.sin(ang)


def noise_normal(seed, streams, k):
    """The standard normals of the streams at step index k: m x 2 x 5, by Box-Muller from
    `noise_uniform` -- rad = sqrt(-2 log(u1)), z[2 j] = rad cos(2 pi u2), z[2 j + 1] = rad sin(2 pi u2)
    -- for (x, y, v, theta, delta) of each vehicle; the sixth is discarded."""
    z = np.stack(_box_muller(noise_uniform(seed, streams, k)), axis=-1)
    return z.reshape(z.shape[0], 2, 6)[..., :NX]


def noise_row(sigma=0.0, bias=0.0, trunc=0.0):
    """One noise row (NOISE_PAR doubles): sigma and bias each one value, five (x, y, v, theta, delta;
    both vehicles) or 2 x 5; trunc 0 for none, else z is clipped to +-trunc before it is scaled."""
    row = np.zeros(NOISE_PAR)
    row[0:10] = np.broadcast_to(np.asarray(sigma, np.float64), (2, NX)).reshape(10)
    row[10:20] = np.broadcast_to(np.asarray(bias, np.float64), (2, NX)).reshape(10)
    row[20] = float(trunc)
    return row


def noise_row_check(row):
    """None when the noise row is good, else what is wrong with it: the library's check."""
    row = np.asarray(row, np.float64).reshape(NOISE_PAR)
    if not np.isfinite(row).all():
        return "every entry finite"
    if not (row[0:10] >= 0.0).all():
        return "sigma >= 0"
    if not row[20] >= 0.0:
        return "trunc 0 (none) or > 0"
    if row[21] != 0.0:
        return "the reserved entry must be 0"
    return None


def _draw_rows(par, width, streams, n):
    """What a wrapper hands the library unchecked: par as rows x width, streams as n int64 or None."""
    rows = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, width))
    if streams is not None:
        streams = np.ascontiguousarray(streams, np.int64).reshape(-1)
        assert streams.shape == (n,), streams.shape
    return rows, streams


def _draw_args(prefix, width, row_check, default_row, n, par, streams, seed, k0):
    """(par, streams, seed, k0) of a noise or delay argument, checked as the library checks: par one
    row or n rows of `width` (None: default_row()), streams n int64 (None: 0 .. n-1)."""
    par = default_row() if par is None else par
    par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, width))
    if par.shape[0] not in (1, n):
        raise ValueError(f"{prefix}: rows must be 1 or n ({n})")
    for k, row in enumerate(par):
        why = row_check(row)
        if why is not None:
            raise ValueError(f"{prefix}: row {k}: {why}")
    streams = np.arange(n, dtype=np.int64) if streams is None else np.ascontiguousarray(streams, np.int64).reshape(-1)
    if streams.shape != (n,) or (streams < 0).any():
        raise ValueError(f"{prefix}: streams must be {n} ids >= 0")
    seed, k0 = int(seed), int(k0)
    if not (0 <= seed < 1 << 64 and 0 <= k0 < NOISE_K_MAX):
        raise ValueError(f"{prefix}: seed a uint64 and 0 <= k0 < 2^31")
    return par, streams, seed, k0


def noise_args(n, par=None, streams=None, seed=0, k0=0):
    """(par, streams, seed, k0) of a noise argument: par one noise row or n rows (None: the zero
    row), as rows x NOISE_PAR; streams n int64 (None: 0 .. n-1); checked as the library checks."""
    return _draw_args("obca.noise", NOISE_PAR, noise_row_check, noise_row, n, par, streams, seed, k0)


def noise_tape(n, cap, par, streams=None, seed=0, k0=0):
    """The disturbance rows k_plan_noise draws, host restatement with the same statements in the
    same order: n x cap x 2 x 5, row [s][i] = bias + sigma * clip(z, +-trunc) with z the normals of
    stream streams[s] (None: s) at step index k0 + i (`noise_normal`) under par (one noise row or
    n).  A pure function of (seed, stream, step index): any row can be drawn alone."""
    n, cap = int(n), int(cap)
    par, streams, seed, k0 = noise_args(n, par, streams, seed, k0)
    if k0 + cap > NOISE_K_MAX:
        raise ValueError("obca.noise_tape: every step index below 2^31")
    P = np.broadcast_to(par, (n, NOISE_PAR))
    sigma, bias, trunc = P[:, 0:10].reshape(n, 2, NX), P[:, 10:20].reshape(n, 2, NX), P[:, 20][:, None, None]
    out = np.zeros((n, cap, 2, NX))
    for i in range(cap):
        z = noise_normal(seed, streams, k0 + i)
        z = np.where(trunc != 0.0, np.minimum(trunc, np.maximum(z, -trunc)), z)
        out[:, i] = bias + sigma * z
    return out


# the communication delay of the plan's exchange (piadmm_obca_delay_plan / piadmm_obca_delay_tau /
# piadmm_obca_delay_exchange, include/piadmm.h): a delay row (DELAY_PAR doubles) is avg[2], std[2],
# tau_max[2], trunc and one reserved zero
DELAY_CALL = 3                        # the Philox call index of the latency: the one the noise leaves free
# the delay items of piadmm_obca_plan_get: name -> (code, dtype) (PIADMM_OBCA_DELAY_GET_*)
DELAY_GET = {"DELAY_PAR": (39, np.float64), "DELAY_TAU": (40, np.float64), "DELAY_STREAMS": (41, np.int64),
             "DELAY_SEED": (42, np.uint64)}


def delay_row(avg=0.0, std=0.0, tau_max=DT, trunc=0.0):
    """One delay row (DELAY_PAR doubles): avg, std and tau_max each one value or one per vehicle;
    trunc 0 for none, else z is clipped to +-trunc before it is scaled.  The default row draws
    tau = 0 always: the plain exchange."""
    row = np.zeros(DELAY_PAR)
    row[0:2] = np.broadcast_to(np.asarray(avg, np.float64), (2,))
    row[2:4] = np.broadcast_to(np.asarray(std, np.float64), (2,))
    row[4:6] = np.broadcast_to(np.asarray(tau_max, np.float64), (2,))
    row[6] = float(trunc)
    return row


def delay_row_check(row):
    """None when the delay row is good, else what is wrong with it: the library's check."""
    row = np.asarray(row, np.float64).reshape(DELAY_PAR)
    if not np.isfinite(row).all():
        return "every entry finite"
    for v in (0, 1):
        if not row[0 + v] >= 0.0:
            return "avg >= 0"
        if not row[2 + v] >= 0.0:
            return "std >= 0"
        if not 0.0 <= row[4 + v] <= DT:
            return "0 <= tau_max <= DT"
    if not row[6] >= 0.0:
        return "trunc 0 (none) or > 0"
    if row[7] != 0.0:
        return "the reserved entry must be 0"
    return None


def delay_args(n, par=None, streams=None, seed=0, k0=0, tape=None):
    """(par, streams, seed, k0, tape) of a delay argument: par one delay row or n rows (None: the
    default row), as rows x DELAY_PAR; streams n int64 (None: 0 .. n-1); tape n x cap x 2 finite
    recorded latencies or None; checked as the library checks."""
    par, streams, seed, k0 = _draw_args("obca.delay", DELAY_PAR, delay_row_check, delay_row, n, par, streams, seed, k0)
    if tape is not None:
        tape = np.ascontiguousarray(tape, np.float64)
        if tape.ndim != 3 or tape.shape[0] != n or tape.shape[2] != 2 or not np.isfinite(tape).all():
            raise ValueError(f"obca.delay: the tape must be {n} x cap x 2 and finite")
    return par, streams, seed, k0, tape


def delay_tau(n, cap, par, streams=None, seed=0, k0=0, tape=None):
    """The latencies k_plan_delay draws, host restatement with the same statements in the same
    order: n x cap x 2, entry [s][i][v] = min(tau_max[v], max(0, tape[s][i][v] + (avg[v] + std[v] *
    clip(z, +-trunc)))) with z = sqrt(-2 log u1) cos(2 pi u2) of the Philox call DELAY_CALL of
    vehicle v of stream streams[s] (None: s) at step index k0 + i (`noise_uniform`), under par (one
    delay row or n); tape the recorded latencies (None: 0).  A pure function of (seed, stream, step
    index); the noise's calls are 0, 1, 2, so the same seed and streams give independent draws."""
    n, cap = int(n), int(cap)
    par, streams, seed, k0, tape = delay_args(n, par, streams, seed, k0, tape)
    if k0 + cap > NOISE_K_MAX:
        raise ValueError("obca.delay_tau: every step index below 2^31")
    if tape is not None and tape.shape[1] != cap:
        raise ValueError(f"obca.delay_tau: the tape must be {n} x {cap} x 2")
    P = np.broadcast_to(par, (n, DELAY_PAR))
    avg, std, tau_max, trunc = P[:, 0:2], P[:, 2:4], P[:, 4:6], P[:, 6][:, None]
    out = np.zeros((n, cap, 2))
    for i in range(cap):
        z = _box_muller(noise_uniform(seed, streams, k0 + i, calls=(DELAY_CALL,))[:, :, 0])[0]
        z = np.where(trunc != 0.0, np.minimum(trunc, np.maximum(z, -trunc)), z)
        x = (0.0 if tape is None else tape[:, i]) + (avg + std * z)
        lo = np.where(x > 0.0, x, 0.0)
        out[:, i] = np.where(lo < tau_max, lo, tau_max)
    return out
