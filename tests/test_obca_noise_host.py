"""Host side of the device-side disturbance noise (piadmm_obca_noise_plan / piadmm_obca_noise_tape,
include/piadmm.h): the header's constants and the bindings, the generator against its known answers,
the statements piadmm.obca.noise_uniform / noise_normal / noise_tape, every refusal of a noise row,
and OBCAPlanner(noise=...) on the CPU (the two launches answered by the restatements,
tests/_obca_edge_ref.OracleBatch).  No kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import _obca_edge_ref as E
import _obca_fleet_cases as F
import _obca_noise_cases as C
from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
SYMBOLS = {"piadmm_obca_noise_tape": 10, "piadmm_obca_noise_plan": 7}


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
    assert _define(src, "PIADMM_OBCA_NOISE_PAR") == obca.NOISE_PAR == _lib.NOISE_PAR == 22
    for name, code in (("PAR", 36), ("STREAMS", 37), ("SEED", 38)):
        assert _define(src, f"PIADMM_OBCA_NOISE_GET_{name}") == obca.NOISE_GET[f"NOISE_{name}"][0] == code
    assert [obca.NOISE_GET[k][1] for k in ("NOISE_PAR", "NOISE_STREAMS", "NOISE_SEED")] == \
        [np.float64, np.int64, np.uint64]
    # the noise items continue piadmm_obca_plan_get's numbering without touching its names
    taken = sorted(v[0] for v in obca.PLAN_GET.values())
    assert sorted(v[0] for v in obca.NOISE_GET.values()) == list(range(taken[-1] + 1, taken[-1] + 4))
    assert not set(obca.NOISE_GET) & set(obca.PLAN_GET)


def test_symbols_are_bound_and_exported_and_the_abi_stays():
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int32_t\s+(piadmm_obca_noise_\w+)\s*\(", src, re.M))
    assert declared == set(SYMBOLS)
    for name, nargs in SYMBOLS.items():
        assert len(bound[name]) == nargs, name
        assert hasattr(lib, name), name
    assert _lib.load().piadmm_abi_version() == 7 and _define(src, "PIADMM_ABI_VERSION") == 7


# ---------------------------------------------------------------------------------------------
# the generator
# ---------------------------------------------------------------------------------------------
def test_philox_known_answers():
    for counter, key, want in C.KNOWN:
        got = obca.philox4x32(np.array(counter, np.uint32), np.array(key, np.uint32))
        assert got.dtype == np.uint32 and got.tolist() == list(want), [hex(int(v)) for v in got]
    # vectorised over leading axes, the key broadcast
    counters = np.array([k[0] for k in C.KNOWN], np.uint64).reshape(3, 1, 4)
    keys = np.array([k[1] for k in C.KNOWN], np.uint64).reshape(3, 1, 2)
    got = obca.philox4x32(np.tile(counters, (1, 2, 1)), keys)
    assert got.shape == (3, 2, 4)
    for i, (_, _, want) in enumerate(C.KNOWN):
        assert got[i, 0].tolist() == got[i, 1].tolist() == list(want)


def test_noise_raw_is_the_counter_layout():
    streams = np.array(C.STREAM_EDGES, np.int64)
    for seed in C.SEEDS:
        for k in (0, 5, 2 ** 31 - 1):
            raw = obca.noise_raw(seed, streams, k)
            assert raw.shape == (4, 2, 3, 4) and raw.dtype == np.uint32
            for s, t in enumerate(C.STREAM_EDGES):
                for v in (0, 1):
                    for j in range(3):
                        want = obca.philox4x32((k, 4 * v + j, t & 0xFFFFFFFF, t >> 32), (seed & 0xFFFFFFFF, seed >> 32))
                        assert raw[s, v, j].tolist() == want.tolist(), (seed, k, t, v, j)
    assert obca.noise_raw(0, [0], 0)[0, 0, 0].tolist() == list(C.KNOWN[0][2])


def test_noise_uniform():
    streams = C.streams_for(129)
    u = obca.noise_uniform(C.SEEDS[1], streams, 7)
    assert u.shape == (129, 2, 3, 2) and u.dtype == np.float64
    assert (u > 0.0).all() and (u < 1.0).all()
    # the integer formula, in Python integers
    raw = obca.noise_raw(C.SEEDS[1], streams, 7)
    for s in (0, 1, 2, 3, 77, 128):
        for v in (0, 1):
            for j in range(3):
                r = [int(x) for x in raw[s, v, j]]
                for h in (0, 1):
                    a = ((r[2 * h] << 32) | r[2 * h + 1]) >> 12
                    assert u[s, v, j, h] == (a + 0.5) * 2.0 ** -52 == (2 * a + 1) / 2 ** 53
    # the extremes of the formula stay strictly inside (0, 1)
    assert 0.0 < 0.5 * 2.0 ** -52 and ((2 ** 52 - 1) + 0.5) * 2.0 ** -52 < 1.0
    # independent of the batch layout: row s of the 129-stream call is the 1-stream call with that id
    for s in (0, 3, 64, 128):
        _bits(u[s:s + 1], obca.noise_uniform(C.SEEDS[1], streams[s:s + 1], 7), f"stream {s} alone")
    _bits(obca.noise_uniform(C.SEEDS[1], streams[::-1].copy(), 7)[::-1], u, "reversed batch")


def test_noise_normal_is_a_normal_generator():
    """2^17 draws at a fixed seed: the mean within 5 standard errors of 0 (1 / sqrt(N)), the variance
    within 5 standard errors of 1 (sqrt(2 / N)).  Deterministic: mean -2.02e-3 (0.73 standard
    errors), variance 0.99804 (0.50 standard errors) on the CPU."""
    m = 2 ** 17 // 10 + 1
    z = obca.noise_normal(12345, np.arange(m, dtype=np.int64), 3).reshape(-1)[:2 ** 17]
    N = z.size
    assert N == 2 ** 17
    mean, var = float(z.mean()), float(z.var())
    print(f"noise_normal over {N} draws: mean {mean:.6e} ({abs(mean) * N ** 0.5:.2f} s.e.), "
          f"variance {var:.6f} ({abs(var - 1.0) / (2.0 / N) ** 0.5:.2f} s.e.)")
    assert abs(mean) <= 5.0 / N ** 0.5
    assert abs(var - 1.0) <= 5.0 * (2.0 / N) ** 0.5
    # the Box-Muller statement, written out for one call
    u = obca.noise_uniform(12345, [9], 3)[0, 1, 2]
    rad = np.sqrt(-2.0 * np.log(u[0]))
    z9 = obca.noise_normal(12345, [9], 3)
    assert z9.shape == (1, 2, 5)
    assert z9[0, 1, 4] == rad * np.cos(2.0 * np.pi * u[1])


# ---------------------------------------------------------------------------------------------
# the tape
# ---------------------------------------------------------------------------------------------
def test_noise_row_layout_and_defaults():
    row = obca.noise_row()
    assert row.shape == (22,) and row.dtype == np.float64 and not row.any()
    row = obca.noise_row(sigma=C.SIGMA, bias=[[1, 2, 3, 4, 5], [6, 7, 8, 9, 10]], trunc=2.5)
    assert row[0:5].tolist() == row[5:10].tolist() == list(C.SIGMA)
    assert row[10:20].tolist() == list(range(1, 11)) and row[20] == 2.5 and row[21] == 0.0
    assert obca.noise_row_check(row) is None and obca.noise_row_check(obca.noise_row()) is None


def test_noise_tape_sigma_zero_is_the_bias_bit_for_bit():
    bias = np.array([[0.1, -0.2, 1e-300, 0.0, 3.0], [1 / 3, -1e300, 5e-324, 0.0, -7.0]])
    tape = obca.noise_tape(4, 3, obca.noise_row(bias=bias), seed=9)
    assert tape.shape == (4, 3, 2, 5)
    # bias + 0 * z: adding a zero of either sign keeps every bit of a bias that is not -0.0
    _bits(tape, np.broadcast_to(bias, (4, 3, 2, 5)), "bias")


def test_noise_tape_statement_trunc_and_k0():
    n, cap = 5, 4
    streams = C.streams_for(n)
    par = np.stack([obca.noise_row(sigma=np.array(C.SIGMA) * (s + 1), bias=0.01 * s) for s in range(n)])
    tape = obca.noise_tape(n, cap, par, streams, seed=C.SEEDS[2], k0=2)
    for i in range(cap):
        z = obca.noise_normal(C.SEEDS[2], streams, 2 + i)
        _bits(tape[:, i], par[:, 10:20].reshape(n, 2, 5) + par[:, 0:10].reshape(n, 2, 5) * z, f"row {i}")
    # one shared row is the n rows; streams=None is 0 .. n-1
    _bits(obca.noise_tape(n, cap, par[1], streams), obca.noise_tape(n, cap, np.tile(par[1], (n, 1)), streams), "shared")
    _bits(obca.noise_tape(n, cap, par[1]), obca.noise_tape(n, cap, par[1], np.arange(n)), "streams=None")
    # k0 shifts
    a, b = obca.noise_tape(n, 2, par, streams, seed=5, k0=3), obca.noise_tape(n, 5, par, streams, seed=5, k0=0)
    _bits(a[:, 0], b[:, 3], "k0 = 3, row 0")
    _bits(a[:, 1], b[:, 4], "k0 = 3, row 1")
    # trunc clips z before the scaling
    unit = obca.noise_tape(64, 2, obca.noise_row(sigma=1.0), seed=5)
    cut = obca.noise_tape(64, 2, obca.noise_row(sigma=1.0, trunc=0.75), seed=5)
    assert (np.abs(unit) > 0.75).any() and (np.abs(unit) < 0.75).any()
    _bits(cut, np.clip(unit, -0.75, 0.75), "trunc")
    scaled = obca.noise_tape(64, 2, obca.noise_row(sigma=2.0, bias=1.0, trunc=0.75), seed=5)
    _bits(scaled, 1.0 + 2.0 * cut, "trunc, then sigma and bias")
    # a trunc so small that everything clips: +-trunc exactly
    ids = C.all_clipped_streams(5, 0, 2, 8, 0.001)
    tiny = obca.noise_tape(8, 2, obca.noise_row(sigma=1.0, trunc=0.001), ids, seed=5)
    assert (np.abs(tiny) == 0.001).all()
    # cap 0
    assert obca.noise_tape(3, 0, par[0]).shape == (3, 0, 2, 5)


def test_row_validation_refuses_every_bad_row():
    for row, word in C.bad_rows():
        why = obca.noise_row_check(row)
        assert why is not None and word in why, (row, why)
        rows = np.stack([obca.noise_row(), obca.noise_row(), row])
        with pytest.raises(ValueError, match="row 2: .*" + word):
            obca.noise_tape(3, 1, rows)
    with pytest.raises(ValueError, match="rows must be 1 or n"):
        obca.noise_tape(3, 1, np.zeros((2, 22)))
    with pytest.raises(ValueError, match="streams"):
        obca.noise_tape(2, 1, obca.noise_row(), streams=[0, -1])
    with pytest.raises(ValueError, match="streams"):
        obca.noise_tape(2, 1, obca.noise_row(), streams=[0, 1, 2])
    with pytest.raises(ValueError, match="k0"):
        obca.noise_tape(2, 1, obca.noise_row(), k0=-1)
    with pytest.raises(ValueError, match="2\\^31"):
        obca.noise_tape(2, 2, obca.noise_row(), k0=2 ** 31 - 1)
    assert obca.noise_tape(2, 1, obca.noise_row(), k0=2 ** 31 - 1).shape == (2, 1, 2, 5)
    with pytest.raises(ValueError, match="seed"):
        obca.noise_tape(2, 1, obca.noise_row(), seed=2 ** 64)


# ---------------------------------------------------------------------------------------------
# the host planner
# ---------------------------------------------------------------------------------------------
def test_host_planner_with_noise_is_the_planner_with_its_tape():
    kw = F.fleet_kwargs([0, 2], 12)
    par = np.stack([obca.noise_row(sigma=C.SIGMA, bias=0.001), obca.noise_row(sigma=np.array(C.SIGMA) * 2, trunc=1.5)])
    noise = dict(par=par, streams=[7, 2 ** 40 + 3], seed=2 ** 63 + 11, k0=5)
    tape = obca.noise_tape(2, 2, par, noise["streams"], noise["seed"], noise["k0"])
    assert tape.any()
    a = obca.OBCAPlanner(E.OracleBatch(), feedback=dict(), noise=noise, **kw)
    b = obca.OBCAPlanner(E.OracleBatch(), feedback=dict(tape=tape), **kw)
    ra, rb = a.run(2), b.run(2)
    _bits(np.asarray(ra.state_record), np.asarray(rb.state_record), "state_record")
    _bits(np.asarray(ra.lambda_record), np.asarray(rb.lambda_record), "lambda_record")
    assert np.array_equal(np.asarray(ra.iter_num_record), np.asarray(rb.iter_num_record))
    # the disturbance moved the vehicles
    plain = obca.OBCAPlanner(E.OracleBatch(), feedback=dict(), **kw).run(1)
    assert not np.array_equal(np.asarray(plain.state_record)[1], np.asarray(ra.state_record)[1])
    # a tape and the noise add up, the tape term first
    extra = np.random.default_rng(3).normal(0.0, 0.01, (2, 2, 2, 5))
    c = obca.OBCAPlanner(E.OracleBatch(), feedback=dict(tape=extra), noise=noise, **kw)
    d = obca.OBCAPlanner(E.OracleBatch(), feedback=dict(tape=extra + tape), **kw)
    c.step()
    d.step()
    _bits(np.stack(c.init_state), np.stack(d.init_state), "tape + noise")
    # attaching feedback again, or detaching it, drops the noise; noise without feedback is refused
    c.set_feedback()
    assert c.noise is None
    c.set_noise(**noise)
    c.clear_noise()
    assert c.noise is None and c.feedback is not None
    c.set_noise(**noise)
    c.clear_feedback()
    assert c.noise is None
    with pytest.raises(_lib.PiadmmError, match="no feedback attached") as e:
        obca.OBCAPlanner(E.OracleBatch(), noise=noise, **kw)
    assert e.value.code == _lib.E_STATE
    with pytest.raises(ValueError, match="row 1: .*sigma"):
        bad = par.copy()
        bad[1, 2] = -1.0
        obca.OBCAPlanner(E.OracleBatch(), feedback=dict(), noise=dict(par=bad), **kw)
