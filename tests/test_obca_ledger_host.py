"""Host side of the tenant ledger (piadmm_obca_ledger_begin / _get / _clear / _stats / _end,
include/piadmm.h): the header's constants and the bindings, the record's layout in NumPy
(piadmm.obca.ledger_unpack), the statistics' view of a set of records (ledger_view, ledger_stats_host)
on records made by hand, and OBCAPlanner(clock=, ledger=True) on the CPU (tests/_obca_edge_ref.OracleBatch):
retiring, admission and the numbering of the ids.  What a record must hold is computed here from the
planner's own run record (piadmm.obca.record_arrays), not by the ledger's code.  No kernel runs here."""
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
SYMBOLS = {"piadmm_obca_ledger_begin": 3, "piadmm_obca_ledger_get": 4, "piadmm_obca_ledger_clear": 1,
           "piadmm_obca_ledger_stats": 7, "piadmm_obca_ledger_end": 1}
# the table of include/piadmm.h: field -> (byte offset, dtype)
LAYOUT = {"id": (0, np.int64), "stream": (8, np.int64), "slot": (16, np.int32), "reason": (20, np.int32),
          "c_first": (24, np.int32), "steps": (28, np.int32), "min_clearance": (32, np.float64),
          "min_clearance_tight": (40, np.float64), "c_min": (48, np.int32), "iter_max": (52, np.int32),
          "iter_sum": (56, np.int64), "local_status_mask": (64, np.int32), "edge_status_mask": (68, np.int32),
          "primal": (72, np.float64), "dual": (80, np.float64), "t_step": (88, np.int32), "reserved": (92, np.int32),
          "state": (96, np.float64)}
PLANT = np.stack([obca.feedback_row(), obca.feedback_row(method=1, n_sub=2, gain_a=0.9),
                  obca.feedback_row(lr=(1.0, 1.1), gain_w=(1.0, 0.95))])
NOISE = np.stack([obca.noise_row(sigma=0.01 * (s + 1), bias=0.001 * s, trunc=1.5 if s else 0.0) for s in range(3)])
DELAY = np.stack([obca.delay_row(avg=(0.03, 0.05), std=0.04 + 0.01 * s, trunc=1.5) for s in range(3)])
STREAMS = np.array([5, 2 ** 32 + 1, 2 ** 63 - 1], np.int64)
SEED, K0 = 2 ** 63 + 12345, 7
LOOP = dict(plant=PLANT, noise=NOISE, delay=DELAY, streams=STREAMS, seed=SEED, k0=K0)
C0, RUNS = (0, 2, 1), (2, 1, 3)                     # three tenants that retire at three different shifts
LEN = tuple(c + 8 + r - 1 for c, r in zip(C0, RUNS))


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
    assert set(re.findall(r"^\s*int32_t\s+(piadmm_obca_ledger_\w+)\s*\(", src, re.M)) == set(SYMBOLS)
    for name, nargs in SYMBOLS.items():
        assert len(bound[name]) == nargs and hasattr(lib, name), name
    assert _lib.load().piadmm_abi_version() == 7 and _define(src, "PIADMM_ABI_VERSION") == 7
    assert _define(src, "PIADMM_OBCA_LEDGER_REC") == _lib.LEDGER_REC == obca.LEDGER_DTYPE.itemsize == 176
    for k, name in enumerate(("COUNT", "RECORDS", "RUNNING", "NEXT_ID")):
        assert _define(src, f"PIADMM_OBCA_LEDGER_GET_{name}") == obca.LEDGER_GET[name][0] == k
    assert obca.LEDGER_GET["COUNT"][1] == np.int32 and obca.LEDGER_GET["NEXT_ID"][1] == np.int64
    assert (obca.LEDGER_RETIRED, obca.LEDGER_ADMITTED, obca.LEDGER_IMPORTED) == (1, 2, 3)


def test_record_layout_is_the_headers_table():
    dt = obca.LEDGER_DTYPE
    assert set(dt.names) == set(LAYOUT)
    for name, (off, kind) in LAYOUT.items():
        assert dt.fields[name][1] == off and dt.fields[name][0].base == np.dtype(kind), name
    assert dt.fields["state"][0].shape == (2, 5) and dt.fields["state"][1] + 80 == 176
    # a blob written word by word, as the device writes it, reads back field by field
    blob = np.zeros(2 * 176, np.uint8)
    for r in range(2):
        w = blob[r * 176:(r + 1) * 176]
        w[0:16].view(np.int64)[:] = (7 + r, 2 ** 40 + r)
        w[16:32].view(np.int32)[:] = (3, 2, 11, 4 + r)
        w[32:48].view(np.float64)[:] = (0.25, 0.125)
        w[48:56].view(np.int32)[:] = (13, 3)
        w[56:64].view(np.int64)[:] = 9
        w[64:72].view(np.int32)[:] = (1, 5)
        w[72:88].view(np.float64)[:] = (1e-3, 2e-3)
        w[88:96].view(np.int32)[:] = (21, 0)
        w[96:176].view(np.float64)[:] = np.arange(10) + r
    rec = obca.ledger_unpack(blob.tobytes())
    assert rec.shape == (2,) and rec["id"].tolist() == [7, 8] and rec["stream"].tolist() == [2 ** 40, 2 ** 40 + 1]
    assert rec["slot"].tolist() == [3, 3] and rec["reason"].tolist() == [2, 2] and rec["c_first"].tolist() == [11, 11]
    assert rec["steps"].tolist() == [4, 5] and rec["min_clearance"].tolist() == [0.25] * 2
    assert rec["min_clearance_tight"].tolist() == [0.125] * 2 and rec["c_min"].tolist() == [13] * 2
    assert rec["iter_max"].tolist() == [3] * 2 and rec["iter_sum"].tolist() == [9] * 2
    assert rec["local_status_mask"].tolist() == [1] * 2 and rec["edge_status_mask"].tolist() == [5] * 2
    assert rec["primal"].tolist() == [1e-3] * 2 and rec["dual"].tolist() == [2e-3] * 2 and rec["t_step"].tolist() == [21] * 2
    _bits(rec["state"][1], (np.arange(10) + 1.0).reshape(2, 5))
    _bits(np.frombuffer(obca.ledger_pack(rec), np.uint8), blob, "ledger_pack")
    with pytest.raises(ValueError, match="multiple of 176"):
        obca.ledger_unpack(blob[:-1])


def _hand_made():
    rec = np.zeros(6, obca.LEDGER_DTYPE)
    rec["id"] = np.arange(6)
    rec["min_clearance"] = [0.5, 0.2, np.inf, 0.2, 1.0, np.nan]          # a tie, and two minima that are not finite
    rec["min_clearance_tight"] = [0.4, 0.0, 0.3, -np.inf, 0.9, 0.3]
    rec["c_min"] = [3, 0, 1, 7, 2, 2]
    rec["iter_max"] = [3, 2, 1, 5, 2, 1]
    rec["iter_sum"] = [7, 2, 1, 2 ** 33, 4, 1]
    rec["local_status_mask"] = [1, 1, 3, 1, 1, 1]
    rec["edge_status_mask"] = [1, 1, 1, 1, 5, 1]
    return rec


def test_view_and_statistics_of_hand_made_records():
    rec = _hand_made()
    clear, summary, iters, mask = obca.ledger_view(rec)
    assert clear.shape == (2, 6, 2) and summary.shape == (6, 4) and iters.shape == (1, 6) and mask.shape == (1, 6, 2)
    _bits(summary[:, 0], rec["min_clearance"])
    _bits(summary[:, 1], rec["c_min"].astype(np.float64))
    _bits(summary[:, 2], rec["min_clearance_tight"])
    _bits(summary[:, 3], rec["iter_sum"].astype(np.float64))
    for row in (0, 1):
        _bits(clear[row, :, 0], rec["min_clearance"])
        _bits(clear[row, :, 1], rec["min_clearance_tight"])
    assert iters.dtype == np.int32 and iters[0].tolist() == [3, 2, 1, 5, 2, 1]
    assert mask.dtype == np.int32 and mask[0].tolist() == [[1, 1], [1, 1], [3, 1], [1, 1], [1, 5], [1, 1]]
    st = obca.ledger_stats_host(rec, [0.3, 0.6], K=4)
    want = obca.fleet_stats_host(clear, summary, iters, mask, edges=[0.3, 0.6], K=4)
    for name in ("hist", "nonfinite", "fleet_min", "fleet_arg", "mask_or", "worst"):
        _bits(getattr(st, name), getattr(want, name), name)
    # and by hand: the tie goes to the earlier record, the minima that are not finite come last and sit in no bin
    assert st.worst.tolist() == [1, 3, 0, 4] and obca.ledger_stats_host(rec, [0.3], K=6).worst.tolist() == [1, 3, 0, 4, 2, 5]
    assert st.hist.tolist() == [[2, 1, 1], [1, 3, 1]] and st.nonfinite.tolist() == [2, 1]
    assert st.fleet_min.tolist() == [0.2, 0.0] and st.fleet_arg.tolist() == [1, 1]
    assert st.iter_sum == 15 + 2 ** 33 and st.iter_max == 5 and st.mask_or.tolist() == [3, 5] and st.flagged == 2
    with pytest.raises(ValueError, match="1 <= K"):
        obca.ledger_stats_host(rec, [0.3], K=7)


# ---------------------------------------------------------------------------------------------
# the host planner
# ---------------------------------------------------------------------------------------------
def _expected(pl, s, c0):
    """What the record of scenario s of a planner that ran from clock c0 holds, from its run record."""
    clear, summary, iters, mask = obca.record_arrays(pl.record, pl.prob)
    R = iters.shape[0]
    return dict(c_first=c0, steps=R, min_clearance=summary[s, 0], c_min=c0 + int(summary[s, 1]),
                min_clearance_tight=summary[s, 2], iter_sum=int(summary[s, 3]), iter_max=int(iters[:, s].max()),
                local_status_mask=int(np.bitwise_or.reduce(mask[:, s, 0])),
                edge_status_mask=int(np.bitwise_or.reduce(mask[:, s, 1])), state=np.asarray(pl.record.state_record)[R, s])


def _same_record(rec, want, what):
    for k, v in want.items():
        _bits(np.asarray(rec[k]), np.asarray(v, rec.dtype.fields[k][0].base).reshape(np.shape(rec[k])), f"{what}: {k}")


@pytest.mark.parametrize("loop", (False, True))
def test_mixed_clocks_retire_into_records_equal_to_each_tenant_alone(loop):
    clock = np.array(list(zip(C0, LEN)), np.int32)
    more = dict(loop=LOOP) if loop else {}
    fleet = obca.OBCAPlanner(E.OracleBatch(), clock=clock, ledger=True, **more, **F.fleet_kwargs([0, 1, 2], 0))
    run0 = fleet.ledger.running.copy()
    assert run0["id"].tolist() == [0, 1, 2] and run0["c_first"].tolist() == list(C0) and not run0["steps"].any()
    assert run0["reason"].tolist() == [0] * 3 and run0["t_step"].tolist() == [-1] * 3
    for s in range(3):
        _bits(run0["state"][s], fleet.init_state[s], "the entry state")
        assert (run0["min_clearance"][s], run0["min_clearance_tight"][s]) == tuple(obca.clearance(fleet.init_state[s], fleet.prob[s]))
    fleet.run(5)
    assert fleet.t_step == 3 and not fleet.clock[:, 2].any()
    rec = fleet.ledger.records
    # scenario 1 retires at the first shift, 0 at the second, 2 at the third
    assert rec["id"].tolist() == [1, 0, 2] and rec["slot"].tolist() == [1, 0, 2] and rec["reason"].tolist() == [1] * 3
    assert rec["t_step"].tolist() == [0, 1, 2] and rec["steps"].tolist() == [1, 2, 3]
    assert rec["stream"].tolist() == ([int(STREAMS[s]) for s in (1, 0, 2)] if loop else [-1] * 3)
    assert fleet.ledger.running["id"].tolist() == [-1] * 3 and fleet.ledger.next_id == 3
    for k, s in enumerate((1, 0, 2)):
        lone_loop = dict(loop=dict(plant=PLANT[s], noise=NOISE[s], delay=DELAY[s], streams=STREAMS[s:s + 1], seed=SEED,
                                   k0=K0)) if loop else {}
        one = obca.OBCAPlanner(E.OracleBatch(), clock=clock[s:s + 1], ledger=True, **lone_loop, **F.fleet_kwargs([s], 0))
        one.run(5)
        assert len(one.record.iter_num_record) == RUNS[s]
        _same_record(rec[k], _expected(one, 0, C0[s]), f"scenario {s} against its run alone")
        lone = one.ledger.records[0]
        for name in ("primal", "dual", "c_min", "min_clearance", "state", "stream", "iter_sum"):
            _bits(rec[k][name], lone[name], f"scenario {s}: {name} of the lone ledger")
        assert rec[k]["primal"] > 0 or rec[k]["dual"] > 0
    # the fleet's own run record says the same of each slot up to its retirement
    assert not np.array_equal(rec["min_clearance"], rec["min_clearance_tight"])


def test_admission_over_an_alive_and_over_a_retired_slot():
    clock = np.array([[0, 51], [2, 10]], np.int32)
    pl = obca.OBCAPlanner(E.OracleBatch(), clock=clock, ledger=True, loop=dict(LOOP, plant=PLANT[:2], noise=NOISE[:2],
                                                                               delay=DELAY[:2], streams=STREAMS[:2]),
                          **F.fleet_kwargs([0, 1], 0))
    pl.step()
    assert pl.clock[:, 2].tolist() == [1, 0] and pl.ledger.records["id"].tolist() == [1]
    before = pl.ledger.running[0].copy()
    assert before["steps"] == 1 and before["id"] == 0
    # slot 1 is retired (appended already: nothing more), slot 0 is alive (reason 2 with the step so far)
    pl.admit([1, 0], [[1, 51], [0, 9]], specs=[F.SPECS[2], F.SPECS[1]], prob=[1, 0], streams=[77, 78])
    rec = pl.ledger.records
    assert rec["id"].tolist() == [1, 0] and rec["reason"].tolist() == [1, 2] and rec["steps"].tolist() == [1, 1]
    assert rec["t_step"].tolist() == [0, 1] and rec["stream"].tolist() == [int(STREAMS[1]), int(STREAMS[0])]
    for name in ("min_clearance", "min_clearance_tight", "c_min", "iter_sum", "state", "primal", "dual", "c_first"):
        _bits(rec[1][name], before[name], name)
    run = pl.ledger.running
    # the new tenants take the next ids in the order of `slots`
    assert run["id"].tolist() == [3, 2] and run["c_first"].tolist() == [0, 1] and run["stream"].tolist() == [78, 77]
    assert not run["steps"].any() and pl.ledger.next_id == 4
    for s in (0, 1):
        _bits(run["state"][s], pl.init_state[s], "the entry state of the admitted tenant")
    pl.run(3)
    # slot 0's new tenant (c0 0, len 9) retires after two steps, at the plan's third shift
    rec = pl.ledger.records
    assert rec["id"].tolist() == [1, 0, 3] and rec["reason"][2] == 1 and rec["steps"][2] == 2 and rec["t_step"][2] == 2
    assert pl.ledger.running["id"].tolist() == [-1, 2] and pl.ledger.running["steps"][1] == 3
    # a full ledger refuses before anything changes
    pl.ledger.cap = 3
    with pytest.raises(ValueError, match="ledger full"):
        pl.admit([1], [[0, 51]], specs=[F.SPECS[0]])
    assert pl.ledger.count == 3 and pl.ledger.running["id"].tolist() == [-1, 2]
    pl.ledger.clear()
    assert pl.ledger.count == 0 and pl.ledger.next_id == 4


def test_ledger_needs_a_clock():
    with pytest.raises(_lib.PiadmmError, match="obca_ledger_begin: no clock attached") as e:
        obca.OBCAPlanner(E.OracleBatch(), ledger=True, **F.fleet_kwargs([0], 0))
    assert e.value.code == _lib.E_STATE


def _host_items(pl):
    """The piadmm_obca_plan_get items of a host planner at a step boundary, as tenant_pack takes them."""
    n = pl.n
    state = np.stack([obca.pack_state(pl.bar_prev[s], pl.init_state[s]) for s in range(n)])
    par = np.zeros((n, obca.FLEET_PAR))
    for j, name in enumerate(obca.FLEET_ROW):
        par[:, j] = getattr(pl, name + "_s")
    lp = pl.loop
    return dict(STATE=state, STATE_PREV=state, CTRL=np.zeros((n, 2, 14)), CTRL_PREV=np.zeros((n, 2, 14)),
                X=np.zeros((n, 2, 8, 5)), LAMBDA=np.stack(pl.lamb_last), PRIMAL=np.zeros(n), DUAL=np.zeros(n),
                PRIMAL_THRES=pl.primal_thres, DUAL_THRES=pl.dual_thres, PAR=par, REF=np.asarray(pl.ref_traj_s),
                ITERS=np.zeros(n, np.int32), STOP=np.ones(n, np.int32), CONVERGE=np.zeros(n, np.int32),
                PROB=np.asarray(pl.prob, np.int32), STATUS_MASK=np.ones((n, 2), np.int32), CLOCK=pl.clock,
                WINDOW=obca.clock_window(pl.ref_traj_s, pl.clock), LOOP_PLANT=lp["plant"], LOOP_NOISE=lp["noise"],
                LOOP_DELAY=lp["delay"], LOOP_TAU=pl.loop_tau(), LOOP_STREAMS=lp["streams"],
                LOOP_SEED=np.array([lp["seed"], lp["k0"], 7], np.uint64))


def test_import_over_an_alive_slot_and_the_cap():
    shared = dict(plant=PLANT[1], noise=NOISE[1], delay=DELAY[1], seed=SEED, k0=K0)      # one row of each kind: it need not travel
    src = obca.OBCAPlanner(E.OracleBatch(), clock=np.array([[2, 51], [0, 51]], np.int32),
                           loop=dict(shared, streams=STREAMS[:2]), **F.fleet_kwargs([1, 2], 0))
    src.step()
    blob = obca.tenant_pack(_host_items(src), [0], 51, loop=True)
    dst = obca.OBCAPlanner(E.OracleBatch(), clock=np.array([[0, 51], [1, 51]], np.int32),
                           loop=dict(shared, streams=np.array([11, 12], np.int64)), **F.fleet_kwargs([0, 3], 0))
    with pytest.raises(_lib.PiadmmError, match="no clock attached"):
        obca.OBCAPlanner(E.OracleBatch(), **F.fleet_kwargs([0], 0)).set_ledger(2)
    dst.set_ledger(cap=1)
    assert dst.ledger.cap == 1 and dst.ledger.running["id"].tolist() == [0, 1]
    dst.step()
    before = dst.ledger.running[1].copy()
    dst.import_tenants([1], blob)
    rec = dst.ledger.records
    assert len(rec) == 1 and (rec["id"][0], rec["slot"][0], rec["reason"][0], rec["steps"][0], rec["t_step"][0]) == (1, 1, 3, 1, 1)
    assert rec["stream"][0] == 12
    for name in ("min_clearance", "min_clearance_tight", "c_min", "c_first", "iter_sum", "state", "primal", "dual"):
        _bits(rec[0][name], before[name], name)
    fresh = dst.ledger.running[1]
    assert (fresh["id"], fresh["c_first"], fresh["steps"], fresh["stream"], fresh["reason"]) == (2, 3, 0, int(STREAMS[0]), 0)
    _bits(fresh["state"], src.init_state[0], "the imported tenant's entry state")
    assert dst.ledger.next_id == 3 and dst.clock[1].tolist() == [3, 51, 1]
    # the row, the thresholds, prob, the reference and the stream id came along: the tenant goes on as at home
    assert dst.prob[1] == src.prob[0] and dst.primal_thres[1] == src.primal_thres[0]
    for name in obca.FLEET_ROW:
        assert getattr(dst, name + "_s")[1] == getattr(src, name + "_s")[0], name
    _bits(dst.loop_tau()[1], src.loop_tau()[0], "the open latency of the imported tenant")
    # the ledger is full: a second import over an alive slot is refused before anything changes, and so is
    # a step that would retire a tenant
    state_before, run_before = [x.copy() for x in dst.init_state], dst.ledger.running.copy()
    with pytest.raises(ValueError, match="ledger full"):
        dst.import_tenants([0], blob)
    assert dst.ledger.count == 1 and dst.ledger.running.tobytes() == run_before.tobytes()
    _bits(np.stack(dst.init_state), np.stack(state_before), "init_state after the refusal")
    src.step()
    dst.step()
    _bits(dst.init_state[1], src.init_state[0], "the imported tenant one step on")
    _bits(dst.lamb_last[1], src.lamb_last[0], "its lamb_bar one step on")
    assert dst.ledger.running["steps"].tolist() == [2, 1]
    dst.clock[0, 1] = dst.clock[0, 0] + 8                # slot 0 retires at the next shift
    t_step, n_rec = dst.t_step, len(dst.record.iter_num_record)
    with pytest.raises(ValueError, match="ledger full"):
        dst.step()
    assert dst.t_step == t_step and len(dst.record.iter_num_record) == n_rec and dst.ledger.count == 1
    dst.clear_ledger()
    assert dst.ledger is None
    dst.step()
    assert dst.clock[:, 2].tolist() == [0, 1]
