"""Host side of the device-resident OBCA-ADMM plan (piadmm_obca_plan_*, include/piadmm.h): the
header's constants against the Python ones, the config struct's layout, the state pack / unpack
round trip and the bindings.  No kernel runs here."""
import ctypes
import os
import re

import numpy as np
from conftest import ROOT

from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
PLAN_SYMBOLS = ("piadmm_obca_plan_cfg_size", "piadmm_obca_plan_begin", "piadmm_obca_plan_iterate",
                "piadmm_obca_plan_shift", "piadmm_obca_plan_step", "piadmm_obca_plan_get", "piadmm_obca_plan_end")


def _define(src, name):
    m = re.search(rf"^#define {name} (-?\d+)\s*$", src, re.M)
    assert m, name
    return int(m.group(1))


def test_header_defines_match_python():
    src = open(HEADER).read()
    assert _define(src, "PIADMM_OBCA_PLAN_STATE") == obca.PLAN_STATE == 556
    assert sum(int(np.prod(s)) for _, s in obca.PLAN_FIELDS) == obca.PLAN_STATE
    codes = {name: int(v) for name, v in re.findall(r"^#define PIADMM_OBCA_PLAN_GET_(\w+) (\d+)\s*$", src, re.M)}
    assert codes == {k: v[0] for k, v in obca.PLAN_GET.items()}
    assert sorted(codes.values()) == list(range(len(codes)))
    for name in ("STATE", "STATE_PREV", "CTRL", "CTRL_PREV", "X", "ITERS", "ACTIVE", "PRIMAL", "DUAL", "STOP",
                 "CONVERGE", "LOCAL_REC", "LOCAL_OUT", "LOCAL_IST", "EDGE_REC", "EDGE_OUT", "EDGE_IST", "T_STEP"):
        assert name in codes, name
    assert _define(src, "PIADMM_OBCA_REC") == obca.REC and _define(src, "PIADMM_OBCA_EDGE_REC") == obca.EDGE_REC
    # the error codes the bindings name
    for name, val in (("ARG", _lib.E_ARG), ("HIP", _lib.E_HIP), ("STATE", _lib.E_STATE), ("NODEV", _lib.E_NODEV)):
        assert re.search(rf"PIADMM_E_{name} = {val},?\s", src), name


def test_config_struct_layout():
    lib = _lib.load()
    assert lib.piadmm_obca_plan_cfg_size() == ctypes.sizeof(_lib.ObcaPlanCfgC) == 8 * 4 + 10 * 8
    # field names and order as the header declares them
    src = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} piadmm_obca_plan_cfg_t;", src).group(1)
    names = [n.strip() for decl in body.split(";") if decl.strip()
             for n in decl.strip().split(None, 1)[1].split(",")]
    assert names == [f for f, _ in _lib.ObcaPlanCfgC._fields_]


def test_every_plan_symbol_is_bound_and_exported():
    bound = {n for n, _, _ in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in PLAN_SYMBOLS:
        assert name in bound, name
        assert hasattr(lib, name), name
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int32_t\s+(piadmm_obca_plan_\w+)\s*\(", src, re.M))
    assert declared == set(PLAN_SYMBOLS)
    assert _lib.load().piadmm_abi_version() == 7


def test_state_round_trip_is_bit_exact():
    for t_step, prob in ((0, 1), (12, 0), (30, 1)):
        bar = obca.seeded_bar_state(t_step, prob)
        init = np.stack([obca.executed_path(v, t_step * obca.DT) for v in (0, 1)])
        vec = obca.pack_state(bar, init)
        assert vec.shape == (obca.PLAN_STATE,) and vec.dtype == np.float64
        bar2, init2 = obca.unpack_state(vec)
        assert set(bar2) == set(bar)
        for k in bar:
            assert bar2[k].shape == bar[k].shape
            assert bar2[k].tobytes() == np.ascontiguousarray(bar[k]).tobytes(), k
        assert init2.tobytes() == init.tobytes()
        assert obca.pack_state(bar2, init2).tobytes() == vec.tobytes()
    # the layout the header states: fields in order, C-contiguous
    vec = np.arange(obca.PLAN_STATE, dtype=np.float64)
    bar, init = obca.unpack_state(vec)
    assert bar["Z_bar"][0, 0, 0] == 0 and bar["A"][0, 0, 0, 0] == 126 and bar["b"][0, 0, 0] == 238
    assert bar["lamb_bar"][0, 0, 0] == 294 and bar["lamb_ij"][0, 0, 0] == 420 and bar["local_x"][0, 0, 0] == 476
    assert init[0, 0] == 546 and init[1, 4] == 555
    assert bar["A"][1, 2, 3, 1] == 126 + (1 * 7 + 2) * 8 + 3 * 2 + 1
