"""The package piadmm.obca against the one module it was: every name the module had still resolves on
the package, every submodule imports alone and none imports inside a function, and the statements that
are now written once (`_draw_args` behind noise_args / delay_args, Box-Muller behind noise_tape /
delay_tau) give what the two copies gave, bit for bit.  The expected arguments come from the module's
own statements, kept below as `_module_noise_args` / `_module_delay_args`; the expected draws are bytes
recorded from the module (tests/golden/obca_draws.npz: noise_tape and delay_tau of the `_noise_case` /
`_delay_case` arguments).  No kernel runs here and libpiadmm.so is not loaded."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from conftest import ROOT

import _obca_delay_cases as D
import _obca_noise_cases as C
from piadmm import obca

PKG = os.path.dirname(obca.__file__)
MODULES = sorted(f[:-3] for f in os.listdir(PKG) if f.endswith(".py") and f != "__init__.py")
GOLDEN = os.path.join(ROOT, "tests", "golden", "obca_draws.npz")

# sorted(k for k, v in vars(piadmm.obca).items() if not isinstance(v, types.ModuleType)) of the module,
# without the dunder names
SURFACE = """
AVG_DELAY DELAY_CALL DELAY_GET DELAY_PAR DELAY_PROB DT DUAL_PAR DUAL_ROW EDGE_OUT EDGE_REC EDGE_WRITES_ITERATE
FEEDBACK_N_SUB_MAX FEEDBACK_PAR FEEDBACK_ROW FLEET_PAR FLEET_ROW LENGTH MAX_STEER MID_LAMB_IJ NE NL NOISE_GET
NOISE_K_MAX NOISE_PAR NT NU NX N_HORZ OBCABatch OBCADevicePlanner OBCAEdgeResult OBCAFleetStats OBCAPlanner OBCAResult
OBCARunRecord OBCATrace ORDER_CLAMP OUT OvertakeSpec PLAN_FIELDS PLAN_GET PLAN_STATE REC STATS_EDGES STATS_WORST STATUS
STATUS_CONVERGED TENANT_ABI TENANT_F64 TENANT_F64_LAW TENANT_HEADER TENANT_INTS TENANT_INT_FIELDS TENANT_MAGIC
TRACE_GET TRACE_LAMBDA T_PERIOD VAR_DELAY WIDTH _DUAL_DEFAULT _EO_COST _EO_DRES _EO_LBN _EO_YBND _EO_YEQ _EO_YIN _EO_Z
_EO_ZB _E_LB _E_LIJ _E_LX _E_PAR _FEEDBACK_DEFAULT _FLEET_INTS _O_AO _O_BO _O_INIT _O_LB _O_LIJ _O_PAR _O_REF _O_ZB
_PHILOX_M _PHILOX_W _TENANT_SHAPES _U32 _box_vertex _per_scenario _plant_rhs _scenario_refs _spec _spec_of _stats_call
_stats_edges _stats_first _tenant_row_check annotations as_written_problem bar_state_update box_clearance
check_converge clearance clock_rows clock_tick clock_window create_bar_state delay_args delay_row delay_row_check
delay_tau dual_row dual_rows edge_record edge_unpack executed_path feedback_args feedback_row feedback_row_check
fleet_stats_host halfspaces iterate_next_state lambda_update lambda_update_pi local_record local_z noise_args
noise_normal noise_raw noise_row noise_row_check noise_tape noise_uniform overtaking_fleet overtaking_problem pack
pack_state philox4x32 plan_order plan_work propagate record_arrays ref_traj_gen scenario_batch seeded_bar_state
separating_duals shift_dual stale_states stats_order tenant_layout tenant_pack tenant_unpack trace_gather_layout
trace_gather_pack trace_gather_unpack unpack unpack_state vehicle_box
""".split()

N = 3
STREAMS = np.array([2 ** 32 + 5, 2 ** 40 + 1, 2 ** 63 - 1], np.int64)      # explicit 64-bit ids above 2^32
SEED, K0 = 2 ** 63 + 12345, 7


def _noise_rows(each):
    rows = [obca.noise_row(sigma=C.SIGMA, bias=0.01 * (s + 1), trunc=1.5 + 0.25 * s) for s in range(N)]
    return np.stack(rows) if each else rows[0]


def _delay_rows(each):
    rows = [obca.delay_row(avg=(0.03 + 0.01 * s, 0.04), std=(0.02, 0.03 + 0.005 * s), tau_max=(obca.DT, 0.08),
                           trunc=1.25 + 0.5 * s) for s in range(N)]
    return np.stack(rows) if each else rows[0]


def _delay_tape(cap=2):
    return 0.002 * np.arange(N * cap * 2, dtype=np.float64).reshape(N, cap, 2) - 0.005


def _noise_case():
    return (N, 2, _noise_rows(True), STREAMS, SEED, K0)


def _delay_case():
    return (N, 2, _delay_rows(True), STREAMS, SEED, K0, _delay_tape())


def _module_noise_args(n, par=None, streams=None, seed=0, k0=0):
    """noise_args as the module had it."""
    par = obca.noise_row() if par is None else par
    par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, obca.NOISE_PAR))
    if par.shape[0] not in (1, n):
        raise ValueError(f"obca.noise: rows must be 1 or n ({n})")
    for k, row in enumerate(par):
        why = obca.noise_row_check(row)
        if why is not None:
            raise ValueError(f"obca.noise: row {k}: {why}")
    streams = np.arange(n, dtype=np.int64) if streams is None else np.ascontiguousarray(streams, np.int64).reshape(-1)
    if streams.shape != (n,) or (streams < 0).any():
        raise ValueError(f"obca.noise: streams must be {n} ids >= 0")
    seed, k0 = int(seed), int(k0)
    if not (0 <= seed < 1 << 64 and 0 <= k0 < obca.NOISE_K_MAX):
        raise ValueError("obca.noise: seed a uint64 and 0 <= k0 < 2^31")
    return par, streams, seed, k0


def _module_delay_args(n, par=None, streams=None, seed=0, k0=0, tape=None):
    """delay_args as the module had it."""
    par = obca.delay_row() if par is None else par
    par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, obca.DELAY_PAR))
    if par.shape[0] not in (1, n):
        raise ValueError(f"obca.delay: rows must be 1 or n ({n})")
    for k, row in enumerate(par):
        why = obca.delay_row_check(row)
        if why is not None:
            raise ValueError(f"obca.delay: row {k}: {why}")
    streams = np.arange(n, dtype=np.int64) if streams is None else np.ascontiguousarray(streams, np.int64).reshape(-1)
    if streams.shape != (n,) or (streams < 0).any():
        raise ValueError(f"obca.delay: streams must be {n} ids >= 0")
    seed, k0 = int(seed), int(k0)
    if not (0 <= seed < 1 << 64 and 0 <= k0 < obca.NOISE_K_MAX):
        raise ValueError("obca.delay: seed a uint64 and 0 <= k0 < 2^31")
    if tape is not None:
        tape = np.ascontiguousarray(tape, np.float64)
        if tape.ndim != 3 or tape.shape[0] != n or tape.shape[2] != 2 or not np.isfinite(tape).all():
            raise ValueError(f"obca.delay: the tape must be {n} x cap x 2 and finite")
    return par, streams, seed, k0, tape


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if isinstance(w, np.ndarray):
            assert g.dtype == w.dtype and g.shape == w.shape and g.flags.c_contiguous and g.tobytes() == w.tobytes()
        else:
            assert type(g) is type(w) and g == w


def _refusal(fn, *a):
    with pytest.raises(ValueError) as e:
        fn(*a)
    return str(e.value)


def test_every_name_of_the_module_resolves_on_the_package():
    assert len(SURFACE) == 157 and len(set(SURFACE)) == 157
    missing = [k for k in SURFACE if not hasattr(obca, k)]
    assert not missing, missing
    for k in ("__doc__", "__name__", "__file__"):
        assert getattr(obca, k)
    assert obca.__doc__.startswith("OBCA local subproblem on the GPU") and "Record layout" in obca.__doc__


@pytest.mark.parametrize("mod", MODULES)
def test_submodule_imports_alone(mod):
    pkg_root = os.path.dirname(os.path.dirname(PKG))
    r = subprocess.run([sys.executable, "-c", f"import piadmm.obca.{mod}"], cwd=pkg_root, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_no_import_inside_a_function():
    assert len(MODULES) >= 2
    for mod in MODULES + ["__init__"]:
        with open(os.path.join(PKG, mod + ".py")) as f:
            src = f.read()
        hits = [line for line in src.split("\n") if re.match(r"\s+(from|import) ", line)]
        assert not hits, (mod, hits)


@pytest.mark.parametrize("each", (False, True))
@pytest.mark.parametrize("streams", (None, STREAMS))
def test_draw_args_equal_the_modules_statements(each, streams):
    _same(obca.noise_args(N, _noise_rows(each), streams, SEED, K0), _module_noise_args(N, _noise_rows(each), streams, SEED, K0))
    for tape in (None, _delay_tape()):
        _same(obca.delay_args(N, _delay_rows(each), streams, SEED, K0, tape),
              _module_delay_args(N, _delay_rows(each), streams, SEED, K0, tape))
    _same(obca.noise_args(N), _module_noise_args(N))
    _same(obca.delay_args(N), _module_delay_args(N))


def test_draw_args_refuse_with_the_modules_words():
    bad_noise, bad_delay = list(C.bad_rows()), list(D.bad_rows())
    assert bad_noise and bad_delay
    for row, word in bad_noise:
        for rows in (row, np.stack([obca.noise_row(), row])):
            n = 1 if np.ndim(rows) == 1 else 2
            got = _refusal(obca.noise_args, n, rows)
            assert got == _refusal(_module_noise_args, n, rows) and got.startswith("obca.noise: row ") and word in got
    for row, word in bad_delay:
        for rows in (row, np.stack([obca.delay_row(), row])):
            n = 1 if np.ndim(rows) == 1 else 2
            got = _refusal(obca.delay_args, n, rows)
            assert got == _refusal(_module_delay_args, n, rows) and got.startswith("obca.delay: row ") and word in got
    # the refusals that are not a row's
    rest = ((None, STREAMS[:2]), (None, -STREAMS), (None, None, 1 << 64), (None, None, 0, obca.NOISE_K_MAX),
            (None, None, -1))
    for a in ((_noise_rows(True)[:2],),) + rest:
        assert _refusal(obca.noise_args, N, *a) == _refusal(_module_noise_args, N, *a)
    for a in ((_delay_rows(True)[:2],),) + rest:
        assert _refusal(obca.delay_args, N, *a) == _refusal(_module_delay_args, N, *a)
    for tape in (_delay_tape()[:2], _delay_tape()[:, :, :1], np.full((N, 2, 2), np.nan)):
        a = (N, None, None, 0, 0, tape)
        assert _refusal(obca.delay_args, *a) == _refusal(_module_delay_args, *a) \
            == f"obca.delay: the tape must be {N} x cap x 2 and finite"


def test_draws_equal_the_bytes_the_module_drew():
    want = np.load(GOLDEN)
    for name, got in (("noise_tape", obca.noise_tape(*_noise_case())), ("delay_tau", obca.delay_tau(*_delay_case()))):
        w = want[name]
        assert got.dtype == w.dtype == np.float64 and got.shape == w.shape, (name, got.shape, w.shape)
        assert got.tobytes() == w.tobytes(), (name, np.abs(got - w).max())
    # the cases are not trivial: the truncation clips some draw and the tape moves some latency
    z = np.stack([obca.noise_normal(SEED, STREAMS, K0 + i) for i in range(2)], axis=1)
    assert (np.abs(z) > _noise_rows(True)[:, 20][:, None, None, None]).any()
    assert not np.array_equal(want["delay_tau"], obca.delay_tau(*_delay_case()[:-1]))
    assert (want["delay_tau"] > 0).any() and np.isfinite(want["noise_tape"]).all()
