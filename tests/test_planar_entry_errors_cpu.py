"""What the 2-D point mass's four trajectory entries (trk_scene2d_traj_cost_grad, trk_scene2d_traj_adam_steps,
trk_scene2d_traj_via_cost_grad, trk_scene2d_traj_via_adam_steps) answer to a bad call: the return code and the FULL trk_last_error()
text of every case of the table below, and the early TRK_OK returns.  The entries share their checks (check_traj_call, check_via_call,
check_planar_adam, check_state_buffers in csrc/trk_planar.hip) but not the ORDER in which the checks speak: the two via entries look at
the TrkPlanarAdam / the cost buffers before the objective, the plain ones after it, and the plain Adam entry names a horizon above the
limit only after the alignment rule.  This file holds what a caller sees of that.

tests/golden/planar_entry_errors.json was recorded by running this same table (CASES) against the library built from the commit BEFORE
the entries were given their shared helpers ("Test the Adam and Gauss-Newton IK kernels off the Panda's happy path"), where each entry
still carried its own copy of the checks: {case id: {"rc": code, "error": text, or null where the call returns TRK_OK}}.

As in test_planar_via_cpu.py the scene is a block of zeros that no call below may reach the point of reading, and the buffers are host
memory that is never read.  NO case is a sound call with batch > 0: such a call would reach a launch, and there is no GPU where this
file runs.  Where a value of the table is sound on its own (n_steps = 0, horizon 1 and 256, a null adam_m without an update), it comes
with an empty batch, with a null cost under lr = 0, or with a second fault."""
import ctypes as C
import json
from pathlib import Path

import pytest

from torch_robotics_amd import _abi, _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "planar_entry_errors.json"
NAN, INF = float("nan"), float("inf")

SCENE = (C.c_char * 4096)()                                 # stands for a TrkScene2D*
_BUF = (C.c_char * (1 << 16))()                             # host memory standing for the device buffers and weights, never read
PTR = (C.addressof(_BUF) + 63) & ~63                        # 64-byte aligned, so PTR + 4 and PTR + 8 are the misaligned pointers
OBJ = (1.0, 0.08, 1.0, 1.0)                                 # w_obj, gp.dt, gp.sigma, gp.weight
ADAM = (5e-3, 3, 1, 1)                                      # lr, pin, first_step, n_steps
VIA = (1.0, 5)                                              # w_via, n_interp


def _ref(s):
    return C.byref(s) if s is not None else None


def _objective(o):
    return None if o is None else _abi.PlanarObjective(o[0], 0, _abi.GpPrior(o[1], o[2], o[3]))


def _via_objective(o, v, alpha, beta):
    """o is None: a null TrkPlanarViaObjective"""
    return None if o is None else _abi.PlanarViaObjective(_objective(o), v[0], v[1], alpha, beta)


def cost_grad(trk, s=SCENE, o=OBJ, q=PTR, qd=PTR, batch=2, horizon=8, cost=PTR, gq=PTR, gqd=PTR):
    return trk.trk_scene2d_traj_cost_grad(s, _ref(_objective(o)), q, qd, batch, horizon, cost, gq, gqd, None)


def adam_steps(trk, s=SCENE, o=OBJ, a=ADAM, q=PTR, qd=PTR, am=PTR, av=PTR, batch=2, horizon=8, cost=PTR):
    return trk.trk_scene2d_traj_adam_steps(s, _ref(_objective(o)), _ref(None if a is None else _abi.PlanarAdam(*a)), q, qd, am, av, batch,
                                           horizon, cost, None)


def via_cost_grad(trk, s=SCENE, o=OBJ, v=VIA, alpha=PTR, beta=PTR, q=PTR, qd=PTR, batch=2, horizon=8, cost=PTR, gq=PTR, gqd=PTR):
    return trk.trk_scene2d_traj_via_cost_grad(s, _ref(_via_objective(o, v, alpha, beta)), q, qd, batch, horizon, cost, gq, gqd, None)


def via_adam_steps(trk, s=SCENE, o=OBJ, v=VIA, alpha=PTR, beta=PTR, a=ADAM, q=PTR, qd=PTR, am=PTR, av=PTR, batch=2, horizon=8, cost=PTR):
    return trk.trk_scene2d_traj_via_adam_steps(s, _ref(_via_objective(o, v, alpha, beta)), _ref(None if a is None else _abi.PlanarAdam(*a)),
                                               q, qd, am, av, batch, horizon, cost, None)


ENTRIES = (cost_grad, adam_steps, via_cost_grad, via_adam_steps)
GRAD, LOOP, WITH_VIA = (cost_grad, via_cost_grad), (adam_steps, via_adam_steps), (via_cost_grad, via_adam_steps)


def _table():
    """[(case id, entry, keyword arguments that differ from a sound call)]"""
    t = []

    def add(entry, label, **kw):
        t.append((f"{entry.__name__}: {label}", entry, kw))

    def obj(k, v):
        vals = list(OBJ)
        vals[k] = v
        return tuple(vals)

    def adam(lr=ADAM[0], pin=ADAM[1], first_step=ADAM[2], n_steps=ADAM[3]):
        return (lr, pin, first_step, n_steps)

    # ---- each null argument (cost is nullable in the loops, gq / gqd together in the evaluations: sound calls, not in the table)
    for e in ENTRIES:
        for name in ("s", "o", "q", "qd"):
            add(e, f"null {name}", **{name: None})
    for e in GRAD:
        add(e, "null cost", cost=None)
        add(e, "null gq only", gq=None)
        add(e, "null gqd only", gqd=None)
    for e in LOOP:
        for name in ("a", "am", "av"):
            add(e, f"null {name}", **{name: None})
    for e in WITH_VIA:
        add(e, "null alpha", alpha=None)
        add(e, "null beta", beta=None)
    # ---- non-finite dt, sigma, gp.weight, w_obj, w_via, lr; dt and sigma <= 0
    for e in ENTRIES:
        for k, name in ((1, "dt"), (2, "sigma"), (3, "gp.weight"), (0, "w_obj")):
            for v in (NAN, INF, -INF):
                add(e, f"{name} = {v}", o=obj(k, v))
        for v in (0.0, -0.1):
            add(e, f"dt = {v}", o=obj(1, v))
            add(e, f"sigma = {v}", o=obj(2, v))
    for v in (NAN, INF, -INF):
        for e in WITH_VIA:
            add(e, f"w_via = {v}", v=(v, 5))
        for e in LOOP:
            add(e, f"lr = {v}", a=adam(lr=v))
    # ---- n_steps, first_step, pin; n_steps = 0 is sound (one evaluation), so it comes with a null cost: nothing to do
    for e in LOOP:
        add(e, "n_steps = -1", a=adam(n_steps=-1))
        add(e, "n_steps = 0, null cost", a=adam(n_steps=0), cost=None)
        add(e, "n_steps = 0, misaligned adam_v", a=adam(n_steps=0), av=PTR + 8)
        add(e, "first_step = 0", a=adam(first_step=0))
        add(e, "first_step = -4", a=adam(first_step=-4))
        add(e, "pin = -1", a=adam(pin=-1))
        add(e, "pin = 16", a=adam(pin=16))
    for e in WITH_VIA:
        for n in (0, -1):
            add(e, f"n_interp = {n}", v=(1.0, n))
    # ---- batch and horizon; 1 and 256 are sound, and so is 257 in trk_scene2d_traj_cost_grad: with an empty batch
    for e in ENTRIES:
        add(e, "batch = -1", batch=-1)
        add(e, "batch = 0x80000000", batch=0x80000000)
        add(e, "batch = 2^40", batch=1 << 40)
        for h in (-1, 0):
            add(e, f"horizon = {h}", horizon=h)
        for h in (1, 256):
            add(e, f"horizon = {h}, batch = 0", horizon=h, batch=0)
            add(e, f"horizon = {h}, misaligned qd", horizon=h, qd=PTR + 4)
        add(e, "horizon = 257, batch = 0", horizon=257, batch=0)
    for e in (adam_steps, via_cost_grad, via_adam_steps):
        add(e, "horizon = 257", horizon=257)
    # ---- a misaligned pointer for each aligned argument
    for e in GRAD:
        for name in ("q", "qd", "gq", "gqd"):
            add(e, f"misaligned {name}", **{name: PTR + 4})
    for e in LOOP:
        for name in ("q", "qd"):
            add(e, f"misaligned {name}", **{name: PTR + 4})
        for name in ("am", "av"):
            add(e, f"misaligned {name} (+ 8)", **{name: PTR + 8})
            add(e, f"misaligned {name} (+ 4)", **{name: PTR + 4})
    # ---- two faults at once: the order of the checks
    # the via entries: the TrkPlanarAdam (loop) / the null buffers (evaluation) before check_via_call, the alignment after it
    add(via_adam_steps, "null a + null o", a=None, o=None)
    add(via_adam_steps, "pin = 16 + null s", a=adam(pin=16), s=None)
    add(via_adam_steps, "n_steps = -1 + w_via = nan", a=adam(n_steps=-1), v=(NAN, 5))
    add(via_adam_steps, "lr = inf + horizon = 257", a=adam(lr=INF), horizon=257)
    add(via_adam_steps, "null q + horizon = 257", q=None, horizon=257)
    add(via_adam_steps, "null q + n_interp = 0", q=None, v=(1.0, 0))
    add(via_adam_steps, "null am + dt = nan", am=None, o=obj(1, NAN))
    add(via_adam_steps, "misaligned am + horizon = 257", am=PTR + 8, horizon=257)
    add(via_cost_grad, "null q + null o", q=None, o=None)
    add(via_cost_grad, "null gq only + dt = nan", gq=None, o=obj(1, NAN))
    add(via_cost_grad, "null cost + horizon = 257", cost=None, horizon=257)
    add(via_cost_grad, "misaligned q + n_interp = 0", q=PTR + 4, v=(1.0, 0))
    add(via_cost_grad, "misaligned q + horizon = 257", q=PTR + 4, horizon=257)
    add(via_cost_grad, "misaligned gqd + null s", gqd=PTR + 4, s=None)
    for e in WITH_VIA:
        add(e, "null o + null s", o=None, s=None)
        add(e, "null alpha + horizon = 257", alpha=None, horizon=257)
        add(e, "null beta + sigma = 0", beta=None, o=obj(2, 0.0))
        add(e, "w_via = inf + batch = -1", v=(INF, 5), batch=-1)
    # the plain entries: everything after check_traj_call; the plain loop's horizon limit after the alignment rule
    add(adam_steps, "null a + null s", a=None, s=None)
    add(adam_steps, "pin = 16 + dt = nan", a=adam(pin=16), o=obj(1, NAN))
    add(adam_steps, "null a + batch = 2^40", a=None, batch=1 << 40)
    add(adam_steps, "null a + null q", a=None, q=None)
    add(adam_steps, "first_step = 0 + null q", a=adam(first_step=0), q=None)
    add(adam_steps, "null q + misaligned qd", q=None, qd=PTR + 4)
    add(adam_steps, "null q + horizon = 257", q=None, horizon=257)
    add(adam_steps, "misaligned am + horizon = 257", am=PTR + 8, horizon=257)
    add(adam_steps, "lr = nan + horizon = 257", a=adam(lr=NAN), horizon=257)
    add(cost_grad, "null q + batch = -1", q=None, batch=-1)
    add(cost_grad, "null cost + sigma = 0", cost=None, o=obj(2, 0.0))
    add(cost_grad, "null gq only + w_obj = inf", gq=None, o=obj(0, INF))
    add(cost_grad, "null qd + misaligned q", qd=None, q=PTR + 4)
    add(cost_grad, "misaligned gq + batch = 2^40", gq=PTR + 4, batch=1 << 40)
    # inside check_traj_call, for all four
    for e in ENTRIES:
        add(e, "horizon = 0 + null s", horizon=0, s=None)
        add(e, "batch = -1 + dt = 0", batch=-1, o=obj(1, 0.0))
        add(e, "dt = nan + gp.weight = nan", o=(1.0, NAN, 1.0, NAN))
        add(e, "batch = 2^40 + w_obj = nan", batch=1 << 40, o=obj(0, NAN))
        # the null and alignment rules speak before an empty batch is served
        add(e, "batch = 0 + misaligned q", batch=0, q=PTR + 4)
    for e in GRAD:
        add(e, "batch = 0 + null gq only", batch=0, gq=None)
    for e in LOOP:
        add(e, "batch = 0 + pin = 16", batch=0, a=adam(pin=16))
        add(e, "batch = 0 + misaligned am", batch=0, am=PTR + 8)
        # without an update adam_m / adam_v are not looked at for null -- but still for alignment
        add(e, "lr = 0 + null am + misaligned q", a=adam(lr=0.0), am=None, q=PTR + 4)
        add(e, "lr = 0 + null cost + misaligned av", a=adam(lr=0.0), cost=None, av=PTR + 8)
    # ---- the early TRK_OK returns: an empty batch with and without buffers; no update and no cost to write
    for e in GRAD:
        add(e, "batch = 0", batch=0)
        add(e, "batch = 0, null buffers", batch=0, q=None, qd=None, cost=None, gq=None, gqd=None)
    for e in LOOP:
        add(e, "batch = 0", batch=0)
        add(e, "batch = 0, null buffers", batch=0, q=None, qd=None, am=None, av=None, cost=None)
        add(e, "lr = 0, null cost", a=adam(lr=0.0), cost=None)
        add(e, "lr = 0, null cost, null adam_m and adam_v (no update: not needed)", a=adam(lr=0.0), cost=None, am=None, av=None)
    return t


CASES = _table()


def answer(trk, entry, kw):
    """what a caller sees of one call: the code, and the error text where there is one"""
    assert kw, "a sound call would reach a launch"
    rc = entry(trk, **kw)
    return {"rc": rc, "error": None if rc == _abi.TRK_OK else trk.trk_last_error().decode("utf-8")}


def record(trk, path=GOLDEN):
    """writes the file the tests compare against (run against the library of the commit named above)"""
    Path(path).write_text(json.dumps({cid: answer(trk, e, kw) for cid, e, kw in CASES}, indent=1, sort_keys=True) + "\n")


@pytest.fixture(scope="module")
def trk():
    if not _lib.LIB_PATH.exists():
        _lib.build()
    return _lib.lib()


@pytest.fixture(scope="module")
def golden():
    return json.loads(GOLDEN.read_text())


def test_the_table_and_the_recorded_file_hold_the_same_cases(golden):
    ids = [c[0] for c in CASES]
    assert len(set(ids)) == len(ids) and set(ids) == set(golden)
    codes = {v["rc"] for v in golden.values()}
    assert codes == {_abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED}         # every kind of answer, and no launch
    assert all((v["error"] is None) == (v["rc"] == _abi.TRK_OK) for v in golden.values())
    # a served call is an empty batch, or a loop with neither an update nor a cost to write
    for cid, e, kw in CASES:
        if golden[cid]["rc"] == _abi.TRK_OK:
            assert kw.get("batch") == 0 or (e in LOOP and kw.get("cost", PTR) is None and (kw["a"][0] == 0.0 or kw["a"][3] == 0)), cid
    pairs = [cid for cid, _, kw in CASES if " + " in cid]
    assert len(pairs) >= 10 and all(len(kw) >= 2 or isinstance(kw.get("o"), tuple) for cid, _, kw in CASES if " + " in cid)


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.__name__)
def test_every_bad_call_gets_the_recorded_code_and_text(trk, golden, entry):
    got = {cid: answer(trk, e, kw) for cid, e, kw in CASES if e is entry}
    assert len(got) >= 30
    wrong = {cid: (g, golden[cid]) for cid, g in got.items() if g != golden[cid]}
    assert not wrong, wrong


def test_the_order_in_which_the_checks_speak(golden):
    """the recorded answers of the two-fault cases, by the check that wins"""
    def text(cid):
        return golden[cid]["error"]

    # the via loop: the TrkPlanarAdam first, then the objective (null, prior, via, horizon), then null buffers, then alignment
    assert "null TrkPlanarAdam" in text("via_adam_steps: null a + null o")
    assert "pin in 0 .. 15" in text("via_adam_steps: pin = 16 + null s") and "pin in 0 .. 15" in text("via_adam_steps: n_steps = -1 + w_via = nan")
    assert "pin in 0 .. 15" in text("via_adam_steps: lr = inf + horizon = 257")
    assert "TRK_PLANAR_MAX_HORIZON" in text("via_adam_steps: null q + horizon = 257")
    assert "n_interp >= 1" in text("via_adam_steps: null q + n_interp = 0")
    assert "finite dt > 0" in text("via_adam_steps: null am + dt = nan")
    assert "TRK_PLANAR_MAX_HORIZON" in text("via_adam_steps: misaligned am + horizon = 257")
    # the via evaluation: null buffers first, then the objective, then alignment
    for cid in ("null q + null o", "null gq only + dt = nan", "null cost + horizon = 257"):
        assert "null q / qd / cost, or only one of gq / gqd" in text("via_cost_grad: " + cid)
    assert "n_interp >= 1" in text("via_cost_grad: misaligned q + n_interp = 0")
    assert "TRK_PLANAR_MAX_HORIZON" in text("via_cost_grad: misaligned q + horizon = 257")
    assert "null scene / objective" in text("via_cost_grad: misaligned gqd + null s")
    # the plain loop: the objective, the TrkPlanarAdam, null buffers, alignment, and only then the horizon limit
    assert "null scene / objective" in text("adam_steps: null a + null s") and "finite dt > 0" in text("adam_steps: pin = 16 + dt = nan")
    assert "too large" in text("adam_steps: null a + batch = 2^40")
    assert "null TrkPlanarAdam" in text("adam_steps: null a + null q") and "pin in 0 .. 15" in text("adam_steps: first_step = 0 + null q")
    assert "null q / qd / adam_m / adam_v" in text("adam_steps: null q + misaligned qd")
    assert "null q / qd / adam_m / adam_v" in text("adam_steps: null q + horizon = 257")
    assert "16-byte aligned" in text("adam_steps: misaligned am + horizon = 257")
    assert "pin in 0 .. 15" in text("adam_steps: lr = nan + horizon = 257")
    assert golden["adam_steps: horizon = 257"]["rc"] == golden["adam_steps: horizon = 257, batch = 0"]["rc"] == _abi.TRK_ERR_UNSUPPORTED
    # the plain evaluation: the objective, null buffers, alignment; any horizon
    assert "batch must be >= 0" in text("cost_grad: null q + batch = -1") and "finite dt > 0" in text("cost_grad: null cost + sigma = 0")
    assert "must be finite" in text("cost_grad: null gq only + w_obj = inf")
    assert "null q / qd / cost" in text("cost_grad: null qd + misaligned q")
    assert "too large" in text("cost_grad: misaligned gq + batch = 2^40")
    assert golden["cost_grad: horizon = 257, batch = 0"]["rc"] == _abi.TRK_OK
