"""Host side of the loop (piadmm_obca_loop_plan / _loop_admit / _loop_draw, include/piadmm.h): the closed
loop of a clocked plan, its step index each tenant's own clock.  The header's constants and the
bindings, piadmm.obca.loop_draw against noise_tape / delay_tau, the tenant record's loop section in
NumPy, and OBCAPlanner(clock=, loop=) on the CPU (tests/_obca_edge_ref.OracleBatch) against the
unclocked planner with feedback=, noise= and delay=.  Every comparison is bit for bit, NumPy against
NumPy.  No kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import _obca_edge_ref as E
import _obca_fleet_cases as F
from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
SYMBOLS = {"piadmm_obca_loop_plan": 11, "piadmm_obca_loop_admit": 7, "piadmm_obca_loop_draw": 12}
N, T0 = 3, 12
PLANT = np.stack([obca.feedback_row(), obca.feedback_row(method=1, n_sub=2, gain_a=0.9),
                  obca.feedback_row(lr=(1.0, 1.1), gain_w=(1.0, 0.95))])
NOISE = np.stack([obca.noise_row(sigma=0.01 * (s + 1), bias=0.001 * s, trunc=1.5 if s else 0.0) for s in range(N)])
DELAY = np.stack([obca.delay_row(avg=(0.03, 0.05), std=0.04 + 0.01 * s, trunc=1.5) for s in range(N)])
STREAMS = np.array([5, 2 ** 32 + 1, 2 ** 63 - 1], np.int64)
SEED, K0 = 2 ** 63 + 12345, 7
LOOP = dict(plant=PLANT, noise=NOISE, delay=DELAY, streams=STREAMS, seed=SEED, k0=K0)


def _bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (msg, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), msg


def _define(src, name):
    m = re.search(rf"^#define {name} (-?\d+)\b", src, re.M)
    assert m, name
    return int(m.group(1))


def test_symbols_header_and_items():
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    src = open(HEADER).read()
    assert set(re.findall(r"^\s*int32_t\s+(piadmm_obca_loop_\w+)\s*\(", src, re.M)) == set(SYMBOLS)
    for name, nargs in SYMBOLS.items():
        assert len(bound[name]) == nargs and hasattr(lib, name), name
    assert _lib.load().piadmm_abi_version() == 7 and _define(src, "PIADMM_ABI_VERSION") == 7
    assert _define(src, "PIADMM_OBCA_TENANT_F64_LOOP") == obca.TENANT_F64_LOOP == 50
    names = ("PLANT", "NOISE", "DELAY", "TAU", "STREAMS", "SEED")
    for name in names:
        assert _define(src, f"PIADMM_OBCA_LOOP_GET_{name}") == obca.LOOP_GET[f"LOOP_{name}"][0]
    # right behind the delay's items, and no name of the other dicts
    last = max(v[0] for v in obca.DELAY_GET.values())
    assert [obca.LOOP_GET[f"LOOP_{k}"][0] for k in names] == list(range(last + 1, last + 7)) and last + 1 == 43
    assert not set(obca.LOOP_GET) & (set(obca.PLAN_GET) | set(obca.NOISE_GET) | set(obca.DELAY_GET))
    assert [obca.LOOP_GET[f"LOOP_{k}"][1] for k in names] == [np.float64] * 4 + [np.int64, np.uint64]


@pytest.mark.parametrize("c", (0, 3, 2 ** 30))
def test_loop_draw_is_the_tapes_row_at_each_clock(c):
    n, k0, seed = 5, 11, 2 ** 63 + 9
    streams = np.array([0, 7, 2 ** 32 + 1, 2 ** 40 + 3, 2 ** 63 - 1], np.int64)
    noise = np.stack([obca.noise_row(sigma=0.02 * (s + 1), bias=0.01 * s, trunc=0.0 if s % 2 else 1.25) for s in range(n)])
    delay = np.stack([obca.delay_row(avg=(0.03, 0.04 + 0.005 * s), std=0.03, trunc=2.0) for s in range(n)])
    clocks = np.array([c, c + 1, 0, c + 4, 2], np.int64)
    clock = np.stack((clocks, np.full(n, 51), np.ones(n, np.int64)), axis=1)
    w, tau = obca.loop_draw(n, clock, noise, delay, streams, seed, k0)
    assert w.shape == (n, 2, 5) and tau.shape == (n, 2) and w.any() and tau.any()
    for s in range(n):
        # row [s][c_s] of the tapes that start at k0: drawn there alone, which is the same row
        _bits(w[s], obca.noise_tape(n, 1, noise, streams, seed, k0 + int(clocks[s]))[s, 0], f"w {s}")
        _bits(tau[s], obca.delay_tau(n, 1, delay, streams, seed, k0 + int(clocks[s]))[s, 0], f"tau {s}")
    if c == 3:
        tape, lat = obca.noise_tape(n, 8, noise, streams, seed, k0), obca.delay_tau(n, 8, delay, streams, seed, k0)
        for s in range(n):
            _bits(w[s], tape[s, clocks[s]], f"tape row {s}")
            _bits(tau[s], lat[s, clocks[s]], f"latency row {s}")
    # a shared row, an absent kind, the plain clocks
    w1, tau1 = obca.loop_draw(n, clocks, noise[1], None, streams, seed, k0)
    _bits(w1, obca.loop_draw(n, clock, np.tile(noise[1], (n, 1)), delay, streams, seed, k0)[0], "shared noise row")
    _bits(tau1, np.zeros((n, 2)), "no delay")
    _bits(obca.loop_draw(n, clock, None, delay, streams, seed, k0)[0], np.zeros((n, 2, 5)), "no noise")
    with pytest.raises(ValueError, match="2\\^31"):
        obca.loop_draw(n, clock, noise, delay, streams, seed, 2 ** 31 - 1 - c)


def _items(n, n_ref, flags, rng):
    it = dict(STATE=rng.standard_normal((n, 556)), STATE_PREV=rng.standard_normal((n, 556)),
              CTRL=rng.standard_normal((n, 2, 14)), CTRL_PREV=rng.standard_normal((n, 2, 14)),
              X=rng.standard_normal((n, 2, 8, 5)), LAMBDA=rng.standard_normal((n, 2, 7, 9)), PRIMAL=rng.random(n),
              DUAL=rng.random(n), PRIMAL_THRES=np.full(n, 0.01), DUAL_THRES=np.full(n, 0.02),
              PAR=np.tile([1.0, 0.1, 0.1, 150.0, 20.0, 1e4, 1e5, 1e3, 1e5, 1e3, 2, 60, 4, 1, 0, 0], (n, 1)).astype(float),
              REF=rng.standard_normal((n, 2, n_ref, 5)), ITERS=np.arange(n, dtype=np.int32), STOP=np.ones(n, np.int32),
              CONVERGE=np.zeros(n, np.int32), PROB=np.ones(n, np.int32), STATUS_MASK=np.ones((n, 2), np.int32),
              CLOCK=np.stack((np.arange(n), np.full(n, n_ref), np.ones(n, int)), axis=1).astype(np.int32),
              WINDOW=rng.standard_normal((n, 2, 8, 5)))
    loop = dict(LOOP_PLANT=PLANT[:n], LOOP_TAU=rng.uniform(0.0, obca.DT, (n, 2)), LOOP_STREAMS=STREAMS[:n],
                LOOP_SEED=np.array([SEED, K0, flags], np.uint64))
    if flags & 2:
        loop["LOOP_NOISE"] = NOISE[:n]
    if flags & 4:
        loop["LOOP_DELAY"] = DELAY[0:1]              # one shared row: it goes into every record
    return it, loop


@pytest.mark.parametrize("flags", (1, 3, 5, 7))
def test_tenant_pack_and_unpack_with_the_loop_section(flags):
    n, n_ref, slots = 3, 12, [2, 0]
    it, loop = _items(n, n_ref, flags, np.random.default_rng(flags))
    plain = obca.tenant_pack(it, slots, n_ref, update_lamb_ij=1)
    # without the loop the blob is what it was: the keyword's default, and extra items change nothing
    _bits(obca.tenant_pack(dict(it, **loop), slots, n_ref, update_lamb_ij=1), plain, "default off")
    assert obca.tenant_layout(n_ref)["F"] + 50 == obca.tenant_layout(n_ref, loop=True)["F"]
    assert not plain[44:64].any() and obca.tenant_unpack(plain)["loop"] == 0
    blob = obca.tenant_pack(dict(it, **loop), slots, n_ref, update_lamb_ij=1, loop=True)
    lay, lay0 = obca.tenant_layout(n_ref, loop=True), obca.tenant_layout(n_ref)
    assert len(blob) == 64 + 2 * lay["record_bytes"] and lay["record_bytes"] == lay0["record_bytes"] + 400
    assert all(o % 2 == 0 for name, (o, _) in lay["f64"].items() if name.startswith("LOOP_"))
    hdr = blob[:64].view(np.int32)
    assert hdr[11] == flags and hdr[14] == K0 and hdr[15] == 0
    assert (int(hdr[12]) & 0xFFFFFFFF) | ((int(hdr[13]) & 0xFFFFFFFF) << 32) == SEED
    # the records but for the section are the plain blob's
    body, body0 = blob[64:].reshape(2, -1), plain[64:].reshape(2, -1)
    _bits(body[:, :8 * lay0["F"]], body0[:, :8 * lay0["F"]], "the fp64 section in front")
    _bits(body[:, 8 * lay["F"]:], body0[:, 8 * lay0["F"]:], "the int32 section")
    t = obca.tenant_unpack(blob)
    assert t["loop"] == flags and t["LOOP_SEED"].tolist() == [SEED, K0, flags]
    _bits(t["LOOP_PLANT"], PLANT[slots], "plant")
    _bits(t["LOOP_NOISE"], NOISE[slots] if flags & 2 else np.zeros((2, 22)), "noise")
    _bits(t["LOOP_DELAY"], np.tile(DELAY[0], (2, 1)) if flags & 4 else np.zeros((2, 8)), "delay")
    _bits(t["LOOP_TAU"], loop["LOOP_TAU"][slots], "tau")
    _bits(t["LOOP_STREAMS"], STREAMS[slots], "streams")
    _bits(t["STATE"], it["STATE"][slots], "STATE")
    # the round trip: packing what was unpacked gives the blob
    again = {k: v for k, v in t.items() if isinstance(v, np.ndarray) and k != "WORK"}      # no order: no WORK item
    _bits(obca.tenant_pack(again, [0, 1], n_ref, 1, loop=True), blob, "round trip")


def test_tenant_unpack_refuses_a_bad_loop_section():
    n, n_ref = 2, 10
    it, loop = _items(n, n_ref, 7, np.random.default_rng(0))
    loop["LOOP_DELAY"] = DELAY[:n]

    def blob_with(**change):
        return obca.tenant_pack(dict(it, **dict(loop, **change)), [0, 1], n_ref, loop=True)
    assert obca.tenant_unpack(blob_with())["m"] == 2
    bad = PLANT[:n].copy()
    bad[1, 1] = 65.0
    with pytest.raises(ValueError, match="row 1: plant: .*n_sub"):
        obca.tenant_unpack(blob_with(LOOP_PLANT=bad))
    bad = NOISE[:n].copy()
    bad[0, 3] = -1.0
    with pytest.raises(ValueError, match="row 0: noise: sigma"):
        obca.tenant_unpack(blob_with(LOOP_NOISE=bad))
    bad = DELAY[:n].copy()
    bad[1, 4] = 0.2
    with pytest.raises(ValueError, match="row 1: delay: .*tau_max"):
        obca.tenant_unpack(blob_with(LOOP_DELAY=bad))
    for tau in (-1e-9, np.nextafter(obca.DT, 1.0), np.nan):
        with pytest.raises(ValueError, match="row 1: tau must be in"):
            obca.tenant_unpack(blob_with(LOOP_TAU=np.array([[0.0, obca.DT], [0.05, tau]])))
    with pytest.raises(ValueError, match="row 0: the stream id"):
        obca.tenant_unpack(blob_with(LOOP_STREAMS=np.array([-1, 3], np.int64)))
    # the header: flags without bit 0, unknown bits, a seed without the loop
    for word, val in ((11, 2), (11, 9), (15, 1)):
        blob = blob_with().copy()
        blob[:64].view(np.int32)[word] = val
        with pytest.raises(ValueError, match="bad header"):
            obca.tenant_unpack(blob)
    blob = obca.tenant_pack(it, [0, 1], n_ref).copy()
    blob[:64].view(np.int32)[12] = 5
    with pytest.raises(ValueError, match="bad header"):
        obca.tenant_unpack(blob)


# ---------------------------------------------------------------------------------------------
# the host planner
# ---------------------------------------------------------------------------------------------
def _kw(cases=(0, 1, 2), t0=T0):
    return F.fleet_kwargs(list(cases), t0)


def test_host_planner_clock_at_zero_is_the_old_closed_loop():
    n_ref = 51
    old = obca.OBCAPlanner(E.OracleBatch(), feedback=dict(par=PLANT), noise=dict(par=NOISE, streams=STREAMS, seed=SEED, k0=K0),
                           delay=dict(par=DELAY, streams=STREAMS, seed=SEED, k0=K0), **_kw(t0=0))
    new = obca.OBCAPlanner(E.OracleBatch(), clock=True, loop=LOOP, **_kw(t0=0))
    assert new.clock[:, 0].tolist() == [0, 0, 0] and new.clock[:, 1].tolist() == [n_ref] * 3
    for step in range(2):
        _bits(new.loop_tau(), old.delay_tau(), f"the latencies of step {step}")
        assert new.loop_tau().any()
        old.step()
        new.step()
    _bits(new.loop_tau(), old.delay_tau(), "the latencies of the open step")
    _bits(np.asarray(new.record.state_record), np.asarray(old.record.state_record), "state_record")
    _bits(np.asarray(new.record.lambda_record), np.asarray(old.record.lambda_record), "lambda_record")
    assert [list(i) for i in new.record.iter_num_record] == [list(i) for i in old.record.iter_num_record]
    # the loop is not the open loop
    plain = obca.OBCAPlanner(E.OracleBatch(), clock=True, **_kw(t0=0)).run(1)
    assert not np.array_equal(np.asarray(plain.state_record)[1], np.asarray(new.record.state_record)[1])


def test_host_planner_mixed_clocks_equal_each_scenario_alone():
    c0 = (0, 2, 1)
    clock = np.array([[c, 51] for c in c0], np.int32)
    fleet = obca.OBCAPlanner(E.OracleBatch(), clock=clock, loop=LOOP, **_kw(t0=0))
    tau0 = fleet.loop_tau()
    fleet.run(2)
    states, lamb = np.asarray(fleet.record.state_record), np.asarray(fleet.record.lambda_record)
    for s, c in enumerate(c0):
        draw = dict(streams=STREAMS[s:s + 1], seed=SEED, k0=K0 + c)
        one = obca.OBCAPlanner(E.OracleBatch(), feedback=dict(par=PLANT[s]), noise=dict(par=NOISE[s], **draw),
                               delay=dict(par=DELAY[s], **draw), **F.fleet_kwargs([s], c))
        _bits(tau0[s], one.delay_tau()[0], f"scenario {s}: the first latency")
        one.run(2)
        _bits(states[:, s], np.asarray(one.record.state_record)[:, 0], f"scenario {s}: state_record")
        _bits(lamb[:, s], np.asarray(one.record.lambda_record)[:, 0], f"scenario {s}: lambda_record")
        _bits(fleet.loop_tau()[s], one.delay_tau()[0], f"scenario {s}: the open latency")


def test_host_planner_refusals():
    kw = _kw(t0=0)
    with pytest.raises(_lib.PiadmmError, match="a clock is attached") as e:
        obca.OBCAPlanner(E.OracleBatch(), clock=True, delay=dict(par=DELAY), **kw)
    assert e.value.code == _lib.E_STATE
    with pytest.raises(AssertionError, match="feedback and clock"):
        obca.OBCAPlanner(E.OracleBatch(), clock=True, feedback=dict(), **kw)
    with pytest.raises(_lib.PiadmmError, match="obca_loop_plan: no clock attached") as e:
        obca.OBCAPlanner(E.OracleBatch(), loop=LOOP, **kw)
    assert e.value.code == _lib.E_STATE
    with pytest.raises(_lib.PiadmmError, match="obca_loop_plan: feedback is attached"):
        obca.OBCAPlanner(E.OracleBatch(), feedback=dict(), loop=LOOP, **kw)
    with pytest.raises(_lib.PiadmmError, match="obca_loop_plan: the delay is attached"):
        obca.OBCAPlanner(E.OracleBatch(), delay=dict(), loop=LOOP, **kw)
    bad = PLANT.copy()
    bad[2, 2] = 0.0
    with pytest.raises(ValueError, match="plant row 2: lr, lf"):
        obca.OBCAPlanner(E.OracleBatch(), clock=True, loop=dict(LOOP, plant=bad), **kw)
    with pytest.raises(ValueError, match="row 1: .*std"):
        bad = DELAY.copy()
        bad[1, 3] = -1.0
        obca.OBCAPlanner(E.OracleBatch(), clock=True, loop=dict(LOOP, delay=bad), **kw)
    with pytest.raises(ValueError, match="streams"):
        obca.OBCAPlanner(E.OracleBatch(), clock=True, loop=dict(LOOP, streams=[0, -1, 2]), **kw)
