"""Export and import of running tenants of the device-resident OBCA-ADMM plan (k_plan_export and
k_plan_import in csrc/piadmm_obca_plan_tenant.hip behind piadmm_obca_tenant_export_bytes / _export / _import;
OBCADevicePlanner.export_tenants, import_tenants, from_tenants, compact, save, load).

Bars.  Both kernels are pure copies and a scenario's answers do not depend on its place in a batch
(tests/test_gpu_obca_order.py, tests/test_gpu_obca_clock.py, bit for bit), so every comparison here
is bit-equality with no tolerance: a blob against piadmm.obca.tenant_pack of the plan's own
piadmm_obca_plan_get items, byte for byte; a moved tenant against the plan it left, which runs on
uninterrupted (an export changes nothing); an untouched tenant against a run without the import.

max_admm_iter <= 2 and n_ref = 51 throughout, the fleets of tests/_obca_fleet_cases.py in the mixed
phases of tests/_obca_clock_cases.py."""
import numpy as np
import pytest

import _obca_clock_cases as K
import _obca_dual_cases as C
import _obca_fleet_cases as F
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

SETUP, _bits = P.SETUP, P._bits
N_REF = K.N_REF
MOVED = ("STATE", "STATE_PREV", "X", "CTRL", "ITERS", "PRIMAL", "DUAL", "STATUS_MASK", "LAMBDA", "CLOCK", "WINDOW")
FROZEN = ("STATE", "STATE_PREV", "X", "CTRL", "LAMBDA", "PRIMAL", "DUAL", "WINDOW")
EVERY = MOVED + ("CTRL_PREV", "STOP", "CONVERGE", "T_STEP", "COUNTS", "REF", "PAR", "PRIMAL_THRES", "DUAL_THRES", "PROB")
LAW_ITEMS = ("DUAL_S", "DUAL_D", "DUAL_S_PREV", "DUAL_D_PREV", "DUAL_PAR")


@pytest.fixture(scope="module")
def batches():
    """Three handles: the plan under test, the plan tenants move to, a plan nothing happens to."""
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    hs = [obca.OBCABatch(0) for _ in range(3)]
    yield hs
    for h in hs:
        h.close()


def mixed(n, shift=0, lens=None):
    """(cases, clock rows) of a fleet of n in mixed phases: case (k + shift) % 4, c0 cycling over K.C0."""
    cases = [(k + shift) % 4 for k in range(n)]
    rows = np.array([[K.C0[(k + shift) % 3], N_REF] for k in range(n)], np.int32)
    for k, extra in (lens or {}).items():
        rows[k, 1] = rows[k, 0] + extra
    return cases, rows


def fleet(batch, n, extras=False, shift=0, lens=None, shared_gains=False):
    """A clocked fleet plan of n in mixed phases; with `extras` the dual law (a gains row per scenario,
    or one shared row) and the order."""
    cases, rows = mixed(n, shift, lens)
    kw = dict(dual=C.GAINS if shared_gains else C.fleet_gains(cases), order=True) if extras else {}
    return obca.OBCADevicePlanner(batch, clock=rows, **F.fleet_kwargs(cases, 0), **kw)


def shared(batch, n, extras=False, clock=True, lens=None):
    """A plan of n on one shared reference and one shared row (piadmm_obca_plan_begin)."""
    kw = dict(SETUP, n_scenarios=n, prob=[SETUP["prob"][k % 3] for k in range(n)],
              primal_thres=[SETUP["primal_thres"][k % 3] for k in range(n)],
              dual_thres=[SETUP["dual_thres"][k % 3] for k in range(n)])
    if extras:
        kw.update(dual=C.GAINS, order=True)
    if clock:
        rows = mixed(n, 0, lens)[1]
        kw.update(clock=rows, t_step0=0)
    pl = obca.OBCADevicePlanner(batch, **kw)
    assert not pl.fleet
    return pl


def items_of(pl, extras=None):
    names = EVERY + (LAW_ITEMS if pl.dual_par is not None else ()) + (("WORK",) if pl.order else ())
    if pl._clock is None:
        names = tuple(k for k in names if k not in ("CLOCK", "WINDOW"))
    return {k: pl.get(k) for k in names}


def same_items(a, b, where):
    assert set(a) == set(b), (where, set(a) ^ set(b))
    for k in a:
        _bits(a[k], b[k], f"{k} {where}")


def same_tenant(pa, sa, pb, sb, law, where, keys=MOVED):
    for k in keys + (("DUAL_S", "DUAL_D") if law else ()):
        _bits(pa.get(k)[sa], pb.get(k)[sb], f"{k} of tenant {sa} -> {sb} {where}")


# ---------------------------------------------------------------------------------------------
# 1. the export kernel alone
# ---------------------------------------------------------------------------------------------
RETIRE70 = {3: 8, 10: 9, 33: 8, 64: 9, 69: 9}          # len = c0 + 8 / + 9: retired after one / two steps


@pytest.mark.parametrize("plan", ["fleet", "fleet-law-order", "shared", "shared-law-order", "bare"])
def test_export_alone(batches, plan):
    b = batches[0]
    extras = plan.endswith("law-order")
    if plan == "bare":
        n, sizes = 5, (1, 4, 5)
        pl = shared(b, n, clock=False)
    else:
        n, sizes = 70, (1, 4, 5, 64, 65)
        pl = (fleet if plan.startswith("fleet") else shared)(b, n, extras, lens=RETIRE70)
    pl.run(2)
    t_step = int(pl.get("T_STEP")[0])
    if plan != "bare":
        alive = pl.clock()[:, 2]
        assert t_step == 2 and [int(alive[s]) for s in RETIRE70] == [0] * 5 and alive.sum() == n - 5
    items = pl.tenant_items()
    before = items_of(pl)
    rng = np.random.default_rng(7)
    for m in sizes:
        for order in ("ascending", "reversed", "scattered"):
            slots = {"ascending": np.arange(m), "reversed": np.arange(n - 1, n - 1 - m, -1),
                     "scattered": rng.permutation(n)[:m]}[order]
            if plan != "bare" and m >= 64:
                assert set(RETIRE70) & set(slots.tolist())              # retired tenants export like any other
            blob = pl.export_tenants(slots)
            want = obca.tenant_pack(items, slots, N_REF, update_lamb_ij=0, t_step=t_step)
            assert len(blob) == want.size, (m, order)
            assert blob == want.tobytes(), (plan, m, order)
    t = obca.tenant_unpack(blob)
    assert (t["law"], t["order"]) == (extras, extras)
    if plan == "bare":
        assert t["CLOCK"].tolist() == [[t_step, N_REF, 1]] * sizes[-1]
    same_items(items_of(pl), before, "after the exports: the plan is not changed")
    pl.close()


# ---------------------------------------------------------------------------------------------
# 2. round trip in place
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "law-order"])
def test_round_trip_in_place(batches, extras):
    b, _, twin_h = batches
    n, lens = 5, {3: 9}
    pl, twin = fleet(b, n, extras, lens=lens), fleet(twin_h, n, extras, lens=lens)
    pl.run(2)
    twin.run(2)
    slots = np.arange(n)
    blob = pl.export_tenants(slots)
    pl.import_tenants(slots, blob)
    assert pl.export_tenants(slots) == blob
    assert pl._clock.tolist() == pl.clock().tolist() == twin.clock().tolist() and pl.clock()[3, 2] == 0
    same_items(items_of(pl), items_of(twin), "after the round trip")
    for step in range(2):
        pl.step()
        twin.step()
        same_items(items_of(pl), items_of(twin), f"{step + 1} steps after the round trip")
    pl.close()
    twin.close()


# ---------------------------------------------------------------------------------------------
# 3. migration
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,extras", [(5, False), (5, True), (70, True)], ids=["5", "5-law-order", "70-law-order"])
def test_migration(batches, n, extras):
    ha, hb, hc = batches
    if n == 5:
        nb, src, dst = 8, np.array([4, 0, 2, 1, 3]), np.array([6, 1, 7, 3, 0])
    else:
        rng = np.random.default_rng(11)
        nb, src = 72, rng.permutation(n)[:66]                # across the 64 / 65 lane boundary
        dst = rng.permutation(nb)[:66]
    rest = np.setdiff1d(np.arange(nb), dst)
    assert len(rest) >= 3
    # B without the import: one step, then the two steps the untouched tenants are compared on
    pb = fleet(hc, nb, extras, shift=1)
    pb.run(1)
    untouched = []
    for _ in range(2):
        pb.step()
        untouched.append({k: pb.get(k)[rest] for k in MOVED + (("DUAL_S", "DUAL_D") if extras else ())})
    pb.close()
    pa, pb = fleet(ha, n, extras), fleet(hb, nb, extras, shift=1)
    pa.run(2)
    pb.run(1)
    pb.import_tenants(dst, pa.export_tenants(src))
    same_tenant(pa, src, pb, dst, extras, "at the import", MOVED + ("CTRL_PREV", "STOP", "CONVERGE", "PRIMAL_THRES",
                                                                    "DUAL_THRES", "PROB", "REF", "PAR"))
    if extras:
        _bits(pb.get("DUAL_PAR")[dst], pa.get("DUAL_PAR")[src], "the gains rows travel")
        _bits(pb.get("WORK")[dst], pa.get("WORK")[src], "WORK")
    assert pb.alive().all() and pb._clock.tolist() == pb.clock().tolist()
    for step in range(2):
        pa.step()
        pb.step()
        same_tenant(pa, src, pb, dst, extras, f"{step + 1} steps after the move")
        for k, want in untouched[step].items():
            _bits(pb.get(k)[rest], want, f"{k} of the untouched tenants, {step + 1} steps after the import")
        assert (pb.get("ITERS")[dst] >= 1).all()
    assert int(pb.get("T_STEP")[0]) == 3 and pb.clock()[dst, 0].tolist() == pa.clock()[src, 0].tolist()
    pa.close()
    pb.close()


# ---------------------------------------------------------------------------------------------
# 4. retired tenants and compaction
# ---------------------------------------------------------------------------------------------
def test_retired_tenant_moves_and_stays_frozen(batches):
    ha, hb, _ = batches
    pa, pb = fleet(ha, 5, lens={1: 9}), fleet(hb, 4, shift=2)
    pa.run(2)
    assert pa.clock()[:, 2].tolist() == [1, 0, 1, 1, 1]
    pb.import_tenants([2], pa.export_tenants([1]))
    assert pb.clock()[:, 2].tolist() == [1, 1, 0, 1] and pb.alive().tolist() == [True, True, False, True]
    frozen = {k: pa.get(k)[1] for k in FROZEN}
    for k in FROZEN:
        _bits(pb.get(k)[2], frozen[k], f"{k} of the retired tenant at the import")
    pb.iterate()
    assert pb.get("ACTIVE").tolist() == [0, 1, 3]
    while pb.counts()[1]:
        pb.iterate()
    pb.shift()
    pb.step()
    for k in FROZEN:
        _bits(pb.get(k)[2], frozen[k], f"{k} of the retired tenant two steps later")
    assert pb.get("ITERS")[2] == 0 and not pb.get("STATUS_MASK")[2].any()
    assert pb.clock()[2].tolist() == pa.clock()[1].tolist()
    pa.close()
    pb.close()


@pytest.mark.parametrize("extras", [False, True], ids=["plain", "law-order"])
def test_compact_keeps_exactly_the_alive(batches, extras):
    ha, _, hc = batches
    n, lens = 6, {1: 9, 4: 8}
    for shared_gains in ([False, True] if extras else [False]):
        pl = fleet(ha, n, extras, lens=lens, shared_gains=shared_gains)
        twin = fleet(hc, n, extras, lens=lens, shared_gains=shared_gains)
        pl.run(2)
        twin.run(2)
        small = pl.compact()
        alive = [0, 2, 3, 5]
        assert small.n == 4 and small.compact_slots.tolist() == alive and small.alive().all()
        assert small.t_step == 2 and int(small.get("T_STEP")[0]) == 2
        assert (small.get("DUAL_PAR").shape[0] == (1 if shared_gains else 4)) if extras else small.dual_par is None
        same_tenant(twin, alive, small, np.arange(4), extras, "after compact()")
        for step in range(2):
            small.step()
            twin.step()
            same_tenant(twin, alive, small, np.arange(4), extras, f"{step + 1} steps after compact()")
        small.close()
        twin.close()


# ---------------------------------------------------------------------------------------------
# 5. checkpoint
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", [False, True], ids=["plain", "law-order"])
def test_checkpoint(batches, extras, tmp_path):
    ha, _, hc = batches
    n, lens = 5, {3: 9}
    pl, twin = fleet(ha, n, extras, lens=lens), fleet(hc, n, extras, lens=lens)
    if not extras:
        pl.trace_begin(4)
    pl.run(2)
    twin.run(2)
    path = pl.save(str(tmp_path / "plan"))
    from piadmm import io
    ck = io.load_plan_checkpoint(path)
    assert ck["t_step"] == 2 and ck["attached"] == dict(fleet=True, clock=True, law=extras, order=extras, trace=not extras)
    assert ck["plan_cfg"]["n_scenarios"] == n and ck["plan_cfg"]["n_ref"] == N_REF and ck["dual_par"] is None
    if not extras:
        assert pl.trace_rows() == 2 and pl.trace_get("STATES").shape == (3, n, 2, 5)     # readable on the source
    pl.close()
    fresh = obca.OBCABatch(0)
    try:
        back = obca.OBCADevicePlanner.load(fresh, path)
        assert back.n == n and back.t_step == 2 and back.fleet and back.order == extras
        same_items(items_of(back), items_of(twin), "after load()")
        for step in range(2):
            back.step()
            twin.step()
            same_items(items_of(back), items_of(twin), f"{step + 1} steps after load()")
        assert int(back.get("T_STEP")[0]) == 4
        back.close()
    finally:
        fresh.close()
    twin.close()


# ---------------------------------------------------------------------------------------------
# 6. refusals leave the plan as it was
# ---------------------------------------------------------------------------------------------
def test_refusals(batches):
    ha, hb, _ = batches
    n = 5
    slots = np.arange(n, dtype=np.int32)

    def refused(pl, call, code, text):
        lib, h = pl._lib, pl.batch._h
        before = items_of(pl)
        assert call() == code, (text, lib.piadmm_obca_last_error(h))
        assert text in lib.piadmm_obca_last_error(h), lib.piadmm_obca_last_error(h)
        same_items(items_of(pl), before, f"after the refused call ({text})")

    def exp(pl, sl, nbytes=None):
        sl = np.ascontiguousarray(sl, np.int32)
        size = len(pl.export_tenants(np.arange(len(sl)))) if nbytes is None else nbytes
        out = np.zeros(max(size, 1), np.uint8)
        return pl._lib.piadmm_obca_tenant_export(pl.batch._h, len(sl), _lib.iptr(sl), out.ctypes.data, size)

    def imp(pl, sl, blob):
        sl = np.ascontiguousarray(sl, np.int32)
        blob = np.frombuffer(blob, np.uint8) if isinstance(blob, bytes) else np.ascontiguousarray(blob, np.uint8)
        return pl._lib.piadmm_obca_tenant_import(pl.batch._h, len(sl), _lib.iptr(sl), blob.ctypes.data, blob.nbytes)

    def edited(blob, lay, k, section, word, value):
        bad = np.frombuffer(blob, np.uint8).copy()
        at = 64 + k * lay["record_bytes"]
        if section == "hdr":
            bad[:64].view(np.int32)[word] = value
        elif section == "f64":
            bad[at:at + 8 * lay["F"]].view(np.float64)[word] = value
        else:
            bad[at + 8 * lay["F"]:at + lay["record_bytes"]].view(np.int32)[word] = value
        return bad

    # the blobs: of a plain plan, of one with the law (a row per scenario) and the order
    rich = fleet(hb, n, True)
    rich.run(1)
    blob_rich = rich.export_tenants(slots)
    pl = fleet(ha, n)
    pl.run(1)
    blob = pl.export_tenants(slots)
    lay, lay_rich = obca.tenant_layout(N_REF), obca.tenant_layout(N_REF, True)
    size = ctypes_size(pl, n)
    assert size == len(blob) == 64 + n * lay["record_bytes"]
    # wrong bytes, duplicate or out-of-range slots: both calls
    refused(pl, lambda: exp(pl, slots, size - 8), _lib.E_ARG, b"obca_tenant_export: the blob is")
    refused(pl, lambda: imp(pl, slots, blob[:-8]), _lib.E_ARG, b"obca_tenant_import: the blob is")
    refused(pl, lambda: imp(pl, slots, blob[:40]), _lib.E_ARG, b"shorter than its header")
    for bad_slots, what in (([0, 1, 1, 3, 4], b"slots[2]"), ([0, 1, 2, 3, n], b"slots[4]"), ([-1, 1, 2, 3, 4], b"slots[0]")):
        refused(pl, lambda: exp(pl, bad_slots, size), _lib.E_ARG, b"obca_tenant_export: " + what)
        refused(pl, lambda: imp(pl, bad_slots, blob), _lib.E_ARG, b"obca_tenant_import: " + what)
    refused(pl, lambda: imp(pl, slots[:4], blob), _lib.E_ARG, b"tenants, not m")
    # the header
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 0, "hdr", 0, 0x12345678)), _lib.E_ARG, b"bad magic")
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 0, "hdr", 1, 6)), _lib.E_ARG, b"ABI 6")
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 0, "hdr", 7, lay["F"] + 2)), _lib.E_ARG, b"bad header")
    # n_ref mismatch: a well-formed blob of a plan with references of 20 rows
    t = obca.tenant_unpack(blob)
    short = {k: v for k, v in t.items() if isinstance(v, np.ndarray) and not k.startswith("DUAL_S") and k not in
             ("DUAL_D", "DUAL_D_PREV", "DUAL_PAR", "WORK")}
    short["REF"] = np.ascontiguousarray(t["REF"][:, :, :20])
    short["CLOCK"] = np.tile(np.array([[5, 20, 1]], np.int32), (n, 1))
    refused(pl, lambda: imp(pl, slots, obca.tenant_pack(short, slots, 20)), _lib.E_ARG, b"n_ref mismatch")
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 0, "hdr", 4, 1)), _lib.E_ARG, b"update_lamb_ij mismatch")
    # a bad parameter row, a bad prob, a bad clock row: the row is named
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 2, "f64", 1378, 0.0)), _lib.E_ARG,
            b"obca_tenant_import: row 2: bad parameters")
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 4, "f64", 1378 + 11, 2.5)), _lib.E_ARG,
            b"obca_tenant_import: row 4: 1 <= max_sqp_iter")
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 1, "int", 3, 2)), _lib.E_ARG, b"obca_tenant_import: row 1: prob")
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 3, "int", 8, -1)), _lib.E_ARG, b"obca_tenant_import: row 3: c >= 0")
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 0, "int", 9, 7)), _lib.E_ARG, b"obca_tenant_import: row 0: 8 <= len")
    refused(pl, lambda: imp(pl, slots, edited(blob, lay, 0, "int", 9, N_REF + 1)), _lib.E_ARG, b"row 0: 8 <= len")
    # law or order mismatch, each way
    refused(pl, lambda: imp(pl, slots, blob_rich), _lib.E_STATE, b"the blob carries a dual law")
    refused(rich, lambda: imp(rich, slots, blob), _lib.E_STATE, b"the plan has a dual law attached")
    rich.clear_order()
    refused(rich, lambda: imp(rich, slots, blob_rich), _lib.E_STATE, b"the blob carries the order's record")
    no_order = rich.export_tenants(slots)
    rich.set_order()
    refused(rich, lambda: imp(rich, slots, no_order), _lib.E_STATE, b"the plan has the order attached")
    # through the wrapper the code and the text arrive as a PiadmmError
    with pytest.raises(_lib.PiadmmError, match="the blob carries a dual law") as ei:
        pl.import_tenants(slots, blob_rich)
    assert ei.value.code == _lib.E_STATE
    # with a trace attached; mid-step
    pl.trace_begin(2)
    refused(pl, lambda: imp(pl, slots, blob), _lib.E_STATE, b"a trace is attached")
    assert exp(pl, slots, size) == 0                        # an export works with a trace attached
    pl.trace_end()
    pl.iterate()
    refused(pl, lambda: exp(pl, slots, size), _lib.E_STATE, b"obca_tenant_export: only at a step boundary")
    refused(pl, lambda: imp(pl, slots, blob), _lib.E_STATE, b"obca_tenant_import: only at a step boundary")
    pl.close()
    rich.close()
    # a differing shared gains row
    one = fleet(hb, n, True, shared_gains=True)
    assert one.get("DUAL_PAR").shape == (1, obca.DUAL_PAR)
    refused(one, lambda: imp(one, slots, blob_rich), _lib.E_ARG, b"row 1: the gains row differs from the plan's shared one")   # row 0 is case 0, whose gains are the shared row
    mine = one.export_tenants(slots)
    one.import_tenants(slots, mine)                         # its own row is its own
    refused(one, lambda: imp(one, slots, edited(mine, lay_rich, 3, "f64", lay_rich["f64"]["DUAL_PAR"][0], 0.123)),
            _lib.E_ARG, b"row 3: the gains row differs")
    one.close()
    # without a clock; into a plan that shares one reference
    cases = mixed(n)[0]
    bare = obca.OBCADevicePlanner(ha, **F.fleet_kwargs(cases, 5))
    refused(bare, lambda: imp(bare, slots, blob), _lib.E_STATE, b"obca_tenant_import: no clock attached")
    bare.close()
    sh = shared(ha, n)
    refused(sh, lambda: imp(sh, slots, blob), _lib.E_STATE, b"needs a plan with a reference and a parameter row per scenario")
    sh.close()
    # no plan at all
    lib = ha._lib
    assert imp_raw(lib, ha._h, slots, blob) == _lib.E_STATE and b"no open plan" in lib.piadmm_obca_last_error(ha._h)


def ctypes_size(pl, m):
    import ctypes
    size = ctypes.c_int64()
    assert pl._lib.piadmm_obca_tenant_export_bytes(pl.batch._h, m, ctypes.byref(size)) == 0
    return size.value


def imp_raw(lib, h, slots, blob):
    blob = np.frombuffer(blob, np.uint8)
    return lib.piadmm_obca_tenant_import(h, len(slots), _lib.iptr(slots), blob.ctypes.data, blob.nbytes)
