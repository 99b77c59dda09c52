"""Host side of the export and import of running tenants (piadmm_obca_tenant_export_bytes / _export /
_import, include/piadmm.h): the header's names and the bindings, the NumPy restatement
piadmm.obca.tenant_pack / tenant_unpack round trip, the record layout against the table the header
documents, the refusals of tenant_unpack, and the checkpoint file of piadmm.io.  No kernel runs here."""
import os
import re

import numpy as np
import pytest
from conftest import ROOT

from piadmm import _lib, io, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
TENANT_SYMBOLS = {"piadmm_obca_tenant_export_bytes": 3, "piadmm_obca_tenant_export": 5, "piadmm_obca_tenant_import": 5}
# the table of include/piadmm.h written out: name, first fp64 word, words (R = 10 n_ref)
FIXED = (("STATE", 0, 556), ("STATE_PREV", 556, 556), ("CTRL", 1112, 28), ("CTRL_PREV", 1140, 28), ("X", 1168, 80),
         ("LAMBDA", 1248, 126), ("PRIMAL", 1374, 1), ("DUAL", 1375, 1), ("PRIMAL_THRES", 1376, 1),
         ("DUAL_THRES", 1377, 1), ("PAR", 1378, 16))
LAW = (("DUAL_S", 0, 126), ("DUAL_D", 126, 126), ("DUAL_S_PREV", 252, 126), ("DUAL_D_PREV", 378, 126),
       ("DUAL_PAR", 504, 8))
INTS = (("ITERS", 0, 1), ("STOP", 1, 1), ("CONVERGE", 2, 1), ("PROB", 3, 1), ("STATUS_MASK", 4, 2), ("WORK", 6, 2),
        ("CLOCK", 8, 3))


def items_of(n, n_ref, law, order, clock, seed=0, shared=False):
    """plan_get items of a made-up plan of n scenarios, every value distinct enough to be told apart."""
    rng = np.random.default_rng(seed)
    it = {k: rng.standard_normal((n,) + obca._TENANT_SHAPES[k])
          for k in ("STATE", "STATE_PREV", "CTRL", "CTRL_PREV", "X", "LAMBDA", "PRIMAL", "DUAL")}
    it["PRIMAL_THRES"] = np.where(np.arange(n) % 3 == 0, np.inf, 0.01 + np.arange(n))
    it["DUAL_THRES"] = 0.02 + np.arange(n)
    rows = 1 if shared else n
    par = np.zeros((rows, obca.FLEET_PAR))
    par[:, :10] = 1.0 + rng.random((rows, 10))
    par[:, 10:14] = (2, 60, 4, 1)
    it["PAR"] = par
    it["REF"] = rng.standard_normal((rows, 2, n_ref, 5))
    for k in ("ITERS", "STOP", "CONVERGE"):
        it[k] = rng.integers(0, 5, n).astype(np.int32)
    it["PROB"] = rng.integers(0, 2, n).astype(np.int32)
    it["STATUS_MASK"] = rng.integers(0, 9, (n, 2)).astype(np.int32)
    if law:
        for k in ("DUAL_S", "DUAL_D", "DUAL_S_PREV", "DUAL_D_PREV"):
            it[k] = rng.standard_normal((n, 2, 7, 9))
        it["DUAL_PAR"] = rng.standard_normal((rows, obca.DUAL_PAR))
    if order:
        it["WORK"] = rng.integers(0, 90, (n, 2)).astype(np.int32)
    if clock:
        c = rng.integers(0, n_ref - 7, n)
        it["CLOCK"] = np.stack((c, np.full(n, n_ref), np.ones(n, int)), axis=1).astype(np.int32)
        it["WINDOW"] = rng.standard_normal((n, 2, 8, 5))
    return it


def test_header_names_and_bindings():
    src = open(HEADER).read()
    bound = {name: len(args) for name, _, args in _lib.SYMBOLS}
    for name, n_args in TENANT_SYMBOLS.items():
        assert re.search(rf"^int32_t {name}\(", src, re.M), name
        assert bound.get(name) == n_args, name
    lib = _lib.load()
    for name in TENANT_SYMBOLS:
        assert hasattr(lib, name), name
    for name, val in (("TENANT_MAGIC", obca.TENANT_MAGIC), ("TENANT_HEADER", obca.TENANT_HEADER),
                      ("TENANT_INTS", obca.TENANT_INTS), ("TENANT_F64", obca.TENANT_F64),
                      ("TENANT_F64_LAW", obca.TENANT_F64_LAW)):
        got = re.search(rf"#define PIADMM_OBCA_{name} (\w+)", src)
        assert got and int(got.group(1), 0) == val, name
    for name in ("PRIMAL_THRES", "DUAL_THRES", "PROB", "DUAL_S_PREV", "DUAL_D_PREV"):
        assert re.search(rf"#define PIADMM_OBCA_PLAN_GET_{name} {obca.PLAN_GET[name][0]}\b", src), name
    assert re.search(r"#define PIADMM_ABI_VERSION 7\b", src) and obca.TENANT_ABI == 7
    # without a handle nothing is touched
    assert lib.piadmm_obca_tenant_export_bytes(None, 1, None) == _lib.E_ARG
    assert lib.piadmm_obca_tenant_export(None, 1, None, None, 0) == _lib.E_ARG
    assert lib.piadmm_obca_tenant_import(None, 1, None, None, 0) == _lib.E_ARG


@pytest.mark.parametrize("order", [False, True])
@pytest.mark.parametrize("law", [False, True])
@pytest.mark.parametrize("n_ref", [8, 51])
def test_layout_matches_the_documented_table(n_ref, law, order):
    lay = obca.tenant_layout(n_ref, law)
    R = 10 * n_ref
    want = {name: (o, w) for name, o, w in FIXED}
    want["REF"] = (1394, R)
    want["WINDOW"] = (1394 + R, 80)
    if law:
        want.update({name: (1474 + R + o, w) for name, o, w in LAW})
    assert lay["f64"] == want
    F = (1986 if law else 1474) + R
    assert lay["F"] == F and lay["record_bytes"] == 8 * F + 48 and lay["record_bytes"] % 16 == 0
    assert lay["ints"] == {name: (o, w) for name, o, w in INTS}
    # every segment but the four scalars starts on an even word and has an even length (16-byte copies)
    for name, (o, w) in lay["f64"].items():
        assert w == 1 or (o % 2 == 0 and w % 2 == 0), name
    # the bytes: every field of a packed blob sits where the table says, the header in front
    n, slots = 5, [3, 0, 4]
    it = items_of(n, n_ref, law, order, clock=True)
    blob = obca.tenant_pack(it, slots, n_ref, update_lamb_ij=1)
    assert blob.dtype == np.uint8 and blob.size == 64 + len(slots) * lay["record_bytes"]
    hdr = blob[:64].view(np.int32)
    assert hdr.tolist() == [obca.TENANT_MAGIC, 7, 3, n_ref, 1, int(law), int(order), F, 12, 8 * F + 48, 64, 0, 0, 0, 0, 0]
    for k, s in enumerate(slots):
        rec = blob[64 + k * lay["record_bytes"]:64 + (k + 1) * lay["record_bytes"]]
        f64, ints = rec[:8 * F].view(np.float64), rec[8 * F:].view(np.int32)
        for name, (o, w) in want.items():
            assert f64[o:o + w].tobytes() == np.ascontiguousarray(it[name][s]).tobytes(), (name, s)
        for name, o, w in INTS:
            if name == "WORK" and not order:
                assert not ints[o:o + w].any()
            else:
                assert ints[o:o + w].tolist() == np.asarray(it[name][s]).reshape(-1).tolist(), (name, s)
        assert ints[11] == 0


@pytest.mark.parametrize("clock", [False, True])
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("law,order", [(False, False), (True, True)])
def test_pack_unpack_round_trip(law, order, shared, clock):
    n, n_ref, slots, t_step = 6, 51, [5, 2, 0, 3], 7
    it = items_of(n, n_ref, law, order, clock, seed=1, shared=shared)
    blob = obca.tenant_pack(it, slots, n_ref, t_step=t_step)
    t = obca.tenant_unpack(blob)
    assert (t["m"], t["n_ref"], t["update_lamb_ij"], t["law"], t["order"]) == (4, n_ref, 0, law, order)
    for name in obca.tenant_layout(n_ref, law)["f64"]:
        if name == "WINDOW" and not clock:
            want = np.stack([it["REF"][0 if shared else s][:, t_step:t_step + 8] for s in slots])
        else:
            src = np.asarray(it[name])
            want = np.stack([src[0 if len(src) == 1 and name in ("PAR", "REF", "DUAL_PAR") else s] for s in slots])
        assert t[name].tobytes() == np.ascontiguousarray(want).tobytes(), name
    for name, _, _ in INTS:
        if name == "WORK" and not order:
            assert not t[name].any()
        elif name == "CLOCK" and not clock:
            assert t[name].tolist() == [[t_step, n_ref, 1]] * 4
        else:
            assert t[name].tolist() == it[name][slots].tolist(), name
    # bytes in, the same tenants out; packing what was unpacked gives the same blob
    assert obca.tenant_unpack(blob.tobytes())["STATE"].tobytes() == t["STATE"].tobytes()
    again = {k: v for k, v in t.items() if isinstance(v, np.ndarray)}
    if not law:
        again = {k: v for k, v in again.items() if not k.startswith("DUAL_") or k == "DUAL_THRES"}
    if not order:
        again.pop("WORK")
    assert obca.tenant_pack(again, range(4), n_ref).tobytes() == blob.tobytes()
    # a window past the end of the reference is zeros
    if not clock:
        late = obca.tenant_unpack(obca.tenant_pack(it, slots, n_ref, t_step=n_ref - 7))
        assert not late["WINDOW"].any() and late["CLOCK"].tolist() == [[n_ref - 7, n_ref, 1]] * 4


def test_unpack_refuses_corrupted_and_truncated_blobs():
    n_ref = 51
    it = items_of(4, n_ref, True, True, True, seed=2)
    blob = obca.tenant_pack(it, [0, 1, 2], n_ref)
    lay = obca.tenant_layout(n_ref, True)
    obca.tenant_unpack(blob)
    with pytest.raises(ValueError, match="shorter than its header"):
        obca.tenant_unpack(blob[:40])
    with pytest.raises(ValueError, match="truncated"):
        obca.tenant_unpack(blob[:-8])
    with pytest.raises(ValueError, match="bytes, not"):
        obca.tenant_unpack(np.concatenate((blob, np.zeros(16, np.uint8))))
    for word, val, why in ((0, 0x12345678, "bad magic"), (1, 6, "ABI 6"), (2, 0, "bad header"), (3, 7, "bad header"),
                           (4, 2, "bad header"), (5, 2, "bad header"), (6, -1, "bad header"), (12, 1, "bad header"),
                           (7, lay["F"] - 2, "section sizes"), (8, 11, "section sizes"),
                           (9, lay["record_bytes"] + 16, "section sizes"), (10, 48, "section sizes"),
                           # a count that disagrees with the length; a flag or n_ref that disagrees with the sizes
                           (2, 2, "bytes, not"), (5, 0, "section sizes"), (3, 50, "section sizes")):
        bad = blob.copy()
        bad[:64].view(np.int32)[word] = val
        with pytest.raises(ValueError, match=why):
            obca.tenant_unpack(bad)


def _with(blob, lay, k, section, word, value):
    bad = blob.copy()
    at = 64 + k * lay["record_bytes"]
    if section == "f64":
        bad[at:at + 8 * lay["F"]].view(np.float64)[word] = value
    else:
        bad[at + 8 * lay["F"]:at + lay["record_bytes"]].view(np.int32)[word] = value
    return bad


@pytest.mark.parametrize("k,section,word,value,why", [
    (1, "f64", 1378 + 0, 0.0, "row 1: bad parameters"),          # rho
    (0, "f64", 1378 + 8, -1.0, "row 0: bad parameters"),         # mu_max
    (2, "f64", 1378 + 11, 0.0, "row 2: 1 <= max_sqp_iter"),
    (2, "f64", 1378 + 11, 2.5, "row 2: 1 <= max_sqp_iter"),
    (0, "f64", 1378 + 13, 2.0, "row 0: start 0 or 1"),
    (1, "f64", 1378 + 12, 16.0, "row 1: -1 <= round_decimals"),
    (1, "f64", 1378 + 10, -1.0, "row 1: max_admm_iter"),
    (2, "int", 3, 2, "row 2: prob must be 0 or 1"),
    (0, "int", 8, -1, "row 0: c >= 0"),
    (1, "int", 9, 7, "row 1: 8 <= len <= n_ref"),
    (1, "int", 9, 52, "row 1: 8 <= len <= n_ref"),
])
def test_unpack_refuses_each_bad_row(k, section, word, value, why):
    n_ref = 51
    it = items_of(4, n_ref, False, False, True, seed=3)
    blob = obca.tenant_pack(it, [3, 1, 2], n_ref)
    with pytest.raises(ValueError, match=why):
        obca.tenant_unpack(_with(blob, obca.tenant_layout(n_ref), k, section, word, value))


def test_a_retired_clock_row_is_a_good_row():
    """c + 8 > len is a retired tenant, not a bad one: it unpacks, alive as the record says."""
    n_ref = 51
    it = items_of(3, n_ref, False, False, True, seed=4)
    it["CLOCK"][1] = (13, 20, 0)
    t = obca.tenant_unpack(obca.tenant_pack(it, [0, 1, 2], n_ref))
    assert t["CLOCK"][1].tolist() == [13, 20, 0]


def test_plan_checkpoint_file(tmp_path):
    n_ref = 51
    it = items_of(3, n_ref, True, False, True, seed=5)
    blob = obca.tenant_pack(it, [0, 1, 2], n_ref)
    cfg = dict(n_scenarios=3, t_step0=0, n_ref=n_ref, update_lamb_ij=0)
    gains = np.arange(8.0)
    path = io.save_plan_checkpoint(str(tmp_path / "plan"), blob.tobytes(), 4, cfg,
                                   dict(fleet=True, clock=True, law=True, trace=True), gains)
    assert path.endswith("plan.npz")
    ck = io.load_plan_checkpoint(path)
    assert ck["tenants"].tobytes() == blob.tobytes() and ck["t_step"] == 4 and ck["plan_cfg"] == cfg
    assert ck["attached"] == dict(fleet=True, clock=True, law=True, order=False, trace=True)
    assert ck["dual_par"].tolist() == gains.tolist()
    assert io.load_plan_checkpoint(io.save_plan_checkpoint(str(tmp_path / "b.npz"), blob, 0, cfg, {}))["dual_par"] is None
    # a truncated blob inside a well-formed file is refused on loading
    io.save_plan_checkpoint(str(tmp_path / "cut"), blob[:-16], 4, cfg, {})
    with pytest.raises(ValueError, match="truncated"):
        io.load_plan_checkpoint(str(tmp_path / "cut"))
    np.savez(str(tmp_path / "other.npz"), x=np.zeros(3))
    with pytest.raises(ValueError, match="not a plan checkpoint"):
        io.load_plan_checkpoint(str(tmp_path / "other.npz"))
