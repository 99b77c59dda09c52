"""Host side of the communication delay in the plan's exchange (piadmm_obca_delay_plan /
piadmm_obca_delay_tau / piadmm_obca_delay_exchange, include/piadmm.h): the header's constants and the
bindings, the statements piadmm.obca.delay_tau and stale_states, every refusal of a delay row, the
first-order cancellation the delay tightening was designed for, and OBCAPlanner(delay=...) on the
CPU (the two launches answered by the restatements, tests/_obca_edge_ref.OracleBatch).  No kernel
runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import _obca_delay_cases as C
import _obca_edge_ref as E
import _obca_fleet_cases as F
from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
SYMBOLS = {"piadmm_obca_delay_tau": 11, "piadmm_obca_delay_exchange": 8, "piadmm_obca_delay_plan": 9}


def _bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (msg, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), msg


def _define(src, name):
    m = re.search(rf"^#define {name} (-?\d+)\s*$", src, re.M)
    assert m, name
    return int(m.group(1))


def test_header_constants_match_python():
    src = open(HEADER).read()
    assert _define(src, "PIADMM_OBCA_DELAY_PAR") == obca.DELAY_PAR == _lib.DELAY_PAR == 8
    assert obca.delay_row().shape == (obca.DELAY_PAR,)
    for name, code in (("PAR", 39), ("TAU", 40), ("STREAMS", 41), ("SEED", 42)):
        assert _define(src, f"PIADMM_OBCA_DELAY_GET_{name}") == obca.DELAY_GET[f"DELAY_{name}"][0] == code
    assert [obca.DELAY_GET[k][1] for k in ("DELAY_PAR", "DELAY_TAU", "DELAY_STREAMS", "DELAY_SEED")] == \
        [np.float64, np.float64, np.int64, np.uint64]
    # the delay items continue the numbering behind the noise's without touching any pinned name
    taken = sorted([v[0] for v in obca.PLAN_GET.values()] + [v[0] for v in obca.NOISE_GET.values()])
    assert taken == list(range(len(taken)))
    assert sorted(v[0] for v in obca.DELAY_GET.values()) == list(range(taken[-1] + 1, taken[-1] + 5))
    assert not set(obca.DELAY_GET) & (set(obca.PLAN_GET) | set(obca.NOISE_GET))


def test_symbols_are_bound_and_exported_and_the_abi_stays():
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int32_t\s+(piadmm_obca_delay_\w+)\s*\(", src, re.M))
    assert declared == set(SYMBOLS)
    for name, nargs in SYMBOLS.items():
        assert len(bound[name]) == nargs, name
        assert hasattr(lib, name), name
    assert _lib.load().piadmm_abi_version() == 7 and _define(src, "PIADMM_ABI_VERSION") == 7


# ---------------------------------------------------------------------------------------------
# the latencies
# ---------------------------------------------------------------------------------------------
def test_delay_words_are_the_free_call_of_the_noise_counter():
    streams = np.array(C.STREAM_EDGES, np.int64)
    for seed in C.SEEDS:
        for k in (0, 5, 2 ** 31 - 1):
            raw = obca.noise_raw(seed, streams, k, calls=(obca.DELAY_CALL,))
            assert raw.shape == (4, 2, 1, 4) and raw.dtype == np.uint32
            noise = obca.noise_raw(seed, streams, k)
            for s, t in enumerate(C.STREAM_EDGES):
                for v in (0, 1):
                    want = obca.philox4x32((k, 4 * v + 3, t & 0xFFFFFFFF, t >> 32), (seed & 0xFFFFFFFF, seed >> 32))
                    assert raw[s, v, 0].tolist() == want.tolist(), (seed, k, t, v)
                    # independent of the noise's three calls at the same seed, stream and step
                    for j in range(3):
                        assert raw[s, v, 0].tolist() != noise[s, v, j].tolist(), (seed, k, t, v, j)
    # the generalised noise_raw is the old one at its default calls, call by call
    _bits(obca.noise_raw(7, streams, 3, calls=(0, 1, 2)), obca.noise_raw(7, streams, 3), "default calls")
    _bits(obca.noise_raw(7, streams, 3, calls=(2, 3))[:, :, 0], obca.noise_raw(7, streams, 3)[:, :, 2], "call 2")


def test_delay_tau_is_the_statement():
    n, cap, seed, k0 = 5, 4, C.SEEDS[2], 2
    streams = C.streams_for(n)
    par = np.stack([obca.delay_row(avg=(0.05, 0.03 + 0.005 * s), std=(0.025, 0.01 * s), tau_max=(0.1, 0.08),
                                   trunc=0.0 if s % 2 else 2.0) for s in range(n)])
    tau = obca.delay_tau(n, cap, par, streams, seed, k0)
    assert tau.shape == (n, cap, 2) and tau.dtype == np.float64
    assert (tau >= 0.0).all() and (tau <= par[:, None, 4:6]).all()
    for i in range(cap):
        u = obca.noise_uniform(seed, streams, k0 + i, calls=(3,))[:, :, 0]
        z = np.sqrt(-2.0 * np.log(u[..., 0])) * np.cos((2.0 * np.pi) * u[..., 1])
        trunc = par[:, 6][:, None]
        z = np.where(trunc != 0.0, np.clip(z, -trunc, trunc), z)
        _bits(tau[:, i], np.minimum(par[:, 4:6], np.maximum(0.0, par[:, 0:2] + par[:, 2:4] * z)), f"row {i}")
    # one shared row is the n rows; streams=None is 0 .. n-1; independent of the batch layout
    _bits(obca.delay_tau(n, cap, par[1], streams), obca.delay_tau(n, cap, np.tile(par[1], (n, 1)), streams), "shared")
    _bits(obca.delay_tau(n, cap, par[1]), obca.delay_tau(n, cap, par[1], np.arange(n)), "streams=None")
    for s in (0, 3, 4):
        _bits(obca.delay_tau(1, cap, par[s], streams[s:s + 1], seed, k0), tau[s:s + 1], f"stream {s} alone")
    _bits(obca.delay_tau(n, cap, par[::-1], streams[::-1].copy(), seed, k0)[::-1], tau, "reversed batch")
    # k0 shifts
    a, b = obca.delay_tau(n, 2, par, streams, 5, 3), obca.delay_tau(n, 5, par, streams, 5, 0)
    _bits(a[:, 0], b[:, 3], "k0 = 3, row 0")
    _bits(a[:, 1], b[:, 4], "k0 = 3, row 1")
    assert obca.delay_tau(3, 0, par[0]).shape == (3, 0, 2)


def test_delay_tau_std_zero_clips_trunc_and_tape():
    # std = 0: min(tau_max, avg) bit for bit
    row = obca.delay_row(avg=(1 / 30, 0.09), std=0.0, tau_max=(0.1, 0.07))
    _bits(obca.delay_tau(4, 3, row, seed=9), np.broadcast_to([1 / 30, 0.07], (4, 3, 2)).copy(), "std = 0")
    _bits(obca.delay_tau(4, 3, obca.delay_row(), seed=9), np.zeros((4, 3, 2)), "the default row")
    # both clips are reached and are exact
    wide = obca.delay_tau(256, 2, obca.delay_row(avg=0.05, std=0.05), seed=5)
    assert (wide == 0.0).any() and (wide == obca.DT).any() and ((wide > 0.0) & (wide < obca.DT)).any()
    assert not np.signbit(wide).any()
    low = obca.delay_tau(256, 2, obca.delay_row(avg=0.05, std=0.05, tau_max=0.06), seed=5)
    _bits(low, np.minimum(wide, 0.06), "tau_max")
    # trunc clips z before the scaling
    free = obca.delay_tau(64, 2, obca.delay_row(avg=0.05, std=0.01), seed=5)
    cut = obca.delay_tau(64, 2, obca.delay_row(avg=0.05, std=0.01, trunc=0.75), seed=5)
    lo, hi = 0.05 + 0.01 * -0.75, 0.05 + 0.01 * 0.75
    assert (free < lo).any() and (free > hi).any()
    _bits(cut, np.clip(free, lo, hi), "trunc")
    # a tape adds its term before the clip
    tape = np.random.default_rng(1).uniform(-0.08, 0.08, (64, 2, 2))
    par = obca.delay_row(avg=0.05, std=0.01)
    u = np.stack([obca.noise_uniform(5, np.arange(64), i, calls=(3,))[:, :, 0] for i in range(2)], axis=1)
    z = np.sqrt(-2.0 * np.log(u[..., 0])) * np.cos((2.0 * np.pi) * u[..., 1])
    got = obca.delay_tau(64, 2, par, seed=5, tape=tape)
    _bits(got, np.minimum(obca.DT, np.maximum(0.0, tape + (0.05 + 0.01 * z))), "tape")
    assert (got == 0.0).any() and (got == obca.DT).any()
    # the tape alone under the zero row: clip(tape)
    _bits(obca.delay_tau(64, 2, C.ZERO_ROW, tape=tape), np.clip(tape, 0.0, obca.DT) + 0.0, "zero row + tape")
    # a tape of valid latencies under the zero row is returned bit for bit: the plan given the
    # device's latencies as a tape runs what the plan that draws them runs
    _bits(obca.delay_tau(64, 2, C.ZERO_ROW, tape=got, seed=77), got, "zero row + a tape of latencies")


def test_row_validation_refuses_every_bad_row():
    for row, word in C.bad_rows():
        why = obca.delay_row_check(row)
        assert why is not None and word in why, (row, why)
        rows = np.stack([obca.delay_row(), obca.delay_row(), row])
        with pytest.raises(ValueError, match="row 2: .*" + word):
            obca.delay_tau(3, 1, rows)
    assert obca.delay_row_check(C.UNIT_ROW) is None and obca.delay_row_check(obca.delay_row(tau_max=0.0)) is None
    with pytest.raises(ValueError, match="rows must be 1 or n"):
        obca.delay_tau(3, 1, np.zeros((2, 8)))
    with pytest.raises(ValueError, match="streams"):
        obca.delay_tau(2, 1, obca.delay_row(), streams=[0, -1])
    with pytest.raises(ValueError, match="streams"):
        obca.delay_tau(2, 1, obca.delay_row(), streams=[0, 1, 2])
    with pytest.raises(ValueError, match="k0"):
        obca.delay_tau(2, 1, obca.delay_row(), k0=-1)
    with pytest.raises(ValueError, match="2\\^31"):
        obca.delay_tau(2, 2, obca.delay_row(), k0=2 ** 31 - 1)
    assert obca.delay_tau(2, 1, obca.delay_row(), k0=2 ** 31 - 1).shape == (2, 1, 2)
    with pytest.raises(ValueError, match="seed"):
        obca.delay_tau(2, 1, obca.delay_row(), seed=2 ** 64)
    with pytest.raises(ValueError, match="tape"):
        obca.delay_tau(2, 1, obca.delay_row(), tape=np.full((2, 1, 2), np.nan))
    with pytest.raises(ValueError, match="tape"):
        obca.delay_tau(2, 2, obca.delay_row(), tape=np.zeros((2, 1, 2)))


# ---------------------------------------------------------------------------------------------
# the stale message
# ---------------------------------------------------------------------------------------------
def test_stale_states_edges():
    X = C.exchange_states(5)
    assert (np.signbit(X) & (X == 0.0)).any()
    out0 = obca.stale_states(X, np.zeros((5, 2)))
    _bits(out0, X[:, :, 1:], "tau = 0 is X[1:], a -0.0 included")
    _bits(obca.stale_states(X[1, 1], 0.0), X[1, 1, 1:], "one vehicle, scalar tau")
    # tau = DT: f = 1 exactly, a + (b - a) is X[:-1] to the rounding of the difference and of the sum,
    # each at most half an ulp of the larger operand; exact where the difference is (dyadic states)
    full = obca.stale_states(X, np.full((5, 2), obca.DT))
    assert obca.DT / obca.DT == 1.0
    bound = np.finfo(float).eps * (np.abs(X[:, :, :-1]) + np.abs(X[:, :, 1:]))
    assert (np.abs(full - X[:, :, :-1]) <= bound).all()
    dyadic = np.round(X * 64.0) / 64.0
    _bits(obca.stale_states(dyadic, np.full((5, 2), obca.DT)) + 0.0, dyadic[:, :, :-1] + 0.0, "tau = DT, dyadic states")
    # inside: the statement, entry by entry; theta linearly without a wrap
    tau = C.exchange_taus(5)
    got = obca.stale_states(X, tau)
    for s in range(5):
        for v in (0, 1):
            for t in range(7):
                for j in range(5):
                    a, b = float(X[s, v, t + 1, j]), float(X[s, v, t, j])
                    want = a if tau[s, v] == 0.0 else a + (float(tau[s, v]) / obca.DT) * (b - a)
                    assert got[s, v, t, j] == want and np.signbit(got[s, v, t, j]) == np.signbit(want)
    th = obca.stale_states(X[2, 1], 0.05)[:, 3]
    assert np.abs(th).max() <= np.pi and (np.abs(th) < 1e-12).any()      # across the cut: the plain mean, no wrap
    # one ulp above 0 takes the interpolating branch: f is subnormal, and X[1:] comes back wherever it is not 0
    tiny = obca.stale_states(X, np.full((5, 2), 5e-324))
    there = X[:, :, 1:] != 0.0
    assert there.any() and (~there).any() and np.array_equal(tiny[there], X[:, :, 1:][there])
    assert (np.abs(tiny[~there]) < 1e-300).all()


def test_bar_state_update_with_tau():
    bar = obca.seeded_bar_state(12, 1)
    X = C.exchange_states(1)[0]
    fullx = [np.concatenate([X[v, 1:], np.ones((7, 4))], axis=1) for v in (0, 1)]
    plain = obca.bar_state_update(bar, fullx, prob=1)
    # the new keywords default to the plain update; tau = 0 is the plain update bit for bit
    zero = obca.bar_state_update(bar, fullx, prob=1, tau=[0.0, 0.0], fullX=X)
    for key in plain:
        _bits(zero[key], plain[key], key)
    tau = [0.03, 0.1]
    out = obca.bar_state_update(bar, fullx, prob=1, tau=tau, fullX=X)
    for v in (0, 1):
        st = obca.stale_states(X[v], tau[v])
        _bits(out["local_x"][v], st, "local_x")
        for t in range(7):
            A, b = obca.halfspaces(st[t], 1)
            _bits(out["A"][v, t], A, "A")
            _bits(out["b"][v, t], b, "b")
    for key in ("Z_bar", "lamb_bar", "lamb_ij"):
        _bits(out[key], bar[key], key)
    with pytest.raises(AssertionError):
        obca.bar_state_update(bar, fullx, prob=1, tau=tau)


def test_first_order_cancellation():
    """Why the feature exists: a vehicle on a straight line at constant speed, its message AVG_DELAY
    late.  With prob = 1 the tightened box centre of the stale message is the true centre plus only
    the variance term sigd (VAR_DELAY v c)^2 -- the mean term AVG_DELAY v c puts back exactly what
    the staleness took; with prob = 0 the box lags the true centre by AVG_DELAY v."""
    sig = np.sqrt(obca.DELAY_PROB / (1.0 - obca.DELAY_PROB))
    for v, th in ((20.0, 0.0), (12.5, 0.3), (8.0, -2.0), (0.0, 1.0)):
        c, s = np.cos(th), np.sin(th)
        t = np.arange(8) * obca.DT
        X = np.stack([3.0 + v * c * t, -1.0 + v * s * t, np.full(8, v), np.full(8, th), np.zeros(8)], axis=1)
        st = obca.stale_states(X, obca.AVG_DELAY)
        for k in range(7):
            true = X[k + 1, :2]
            assert np.allclose(st[k, 2:], X[k + 1, 2:], rtol=0, atol=0)          # v, theta, delta are constant
            # prob = 1: the centre the halfspaces are built around, from b = b0 + A (centre)
            A, b = obca.halfspaces(st[k], 1)
            centre = np.linalg.solve(A[:2], (b - np.array([1.75, 1.0, 1.75, 1.0]))[:2])
            var = sig * np.array([(obca.VAR_DELAY * v * c) ** 2, (obca.VAR_DELAY * v * s) ** 2])
            # rounding: a few ulp of the coordinates (|x|, |y| < 20) through the interpolation and the solve
            assert np.abs(centre - (true + var)).max() <= 64 * np.finfo(float).eps * 20.0, (v, th, k)
            # prob = 0: the plain box of the stale state lags by AVG_DELAY v along the heading
            A0, b0 = obca.halfspaces(st[k], 0)
            centre0 = np.linalg.solve(A0[:2], (b0 - np.array([1.75, 1.0, 1.75, 1.0]))[:2])
            lag = true - centre0
            assert abs(lag @ np.array([c, s]) - obca.AVG_DELAY * v) <= 64 * np.finfo(float).eps * 20.0
            assert abs(lag @ np.array([-s, c])) <= 64 * np.finfo(float).eps * 20.0


# ---------------------------------------------------------------------------------------------
# the host planner
# ---------------------------------------------------------------------------------------------
def test_host_planner_with_delay():
    kw = F.fleet_kwargs([0, 2], 12)
    par = np.stack([C.UNIT_ROW, obca.delay_row(avg=0.03, std=0.05, trunc=1.5)])
    delay = dict(par=par, streams=[7, 2 ** 40 + 3], seed=2 ** 63 + 11, k0=5)
    taus = obca.delay_tau(2, 2, par, delay["streams"], delay["seed"], delay["k0"])
    assert taus.any()
    seen = []

    def on_stage(name, inputs, outputs):
        if name == "local":
            seen.append(dict(X=[x.copy() for x in inputs_X(outputs)], scenarios=list(inputs["scenarios"])))
        if name == "exchange":
            seen[-1]["bar"] = outputs["bar"]

    def inputs_X(outputs):
        return outputs["result"].X

    a = obca.OBCAPlanner(E.OracleBatch(), delay=delay, on_stage=on_stage, **kw)
    _bits(a.delay_tau(), taus[:, 0], "the open step's latencies")
    a.step()
    _bits(a.delay_tau(), taus[:, 1], "the next step's latencies")
    # every iterate of step 1 sent the stale states under the step's one latency per vehicle
    assert len(seen) >= 2
    for it in seen:
        for k, s in enumerate(it["scenarios"]):
            for v in (0, 1):
                _bits(it["bar"][k]["local_x"][v], obca.stale_states(it["X"][2 * k + v], taus[s, 0, v]), "local_x sent")
    # the same planner given the latencies as a tape under the zero row
    b = obca.OBCAPlanner(E.OracleBatch(), delay=dict(par=C.ZERO_ROW, tape=taus), **kw)
    a.step()
    b.run(2)
    _bits(np.asarray(a.record.state_record), np.asarray(b.record.state_record), "state_record")
    _bits(np.asarray(a.record.lambda_record), np.asarray(b.record.lambda_record), "lambda_record")
    with pytest.raises(AssertionError, match="latency tape exhausted"):
        b.step()
    # the zero row, and attach then detach, are the plain planner; the delay is not
    plain = obca.OBCAPlanner(E.OracleBatch(), **kw).run(1)
    zero = obca.OBCAPlanner(E.OracleBatch(), delay=dict(), **kw).run(1)
    det = obca.OBCAPlanner(E.OracleBatch(), delay=delay, **kw)
    det.clear_delay()
    assert det.delay is None
    for rec in (zero, det.run(1)):
        _bits(np.asarray(rec.state_record), np.asarray(plain.state_record), "state_record")
        _bits(np.asarray(rec.lambda_record), np.asarray(plain.lambda_record), "lambda_record")
    assert not np.array_equal(np.asarray(plain.lambda_record)[0], np.asarray(a.record.lambda_record)[0])
    # refusals
    with pytest.raises(ValueError, match="row 1: .*std"):
        bad = par.copy()
        bad[1, 3] = -1.0
        obca.OBCAPlanner(E.OracleBatch(), delay=dict(par=bad), **kw)
    with pytest.raises(_lib.PiadmmError, match="a clock is attached") as e:
        obca.OBCAPlanner(E.OracleBatch(), clock=True, delay=delay, **kw)
    assert e.value.code == _lib.E_STATE
