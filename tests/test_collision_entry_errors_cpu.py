"""What the five boolean-mode entries (trk_rollout_collision, trk_rollout_collision_via, trk_rollout_collision_via_flags,
trk_rollout_points_collision, trk_rollout_points_collision_via) answer to a bad call: the return code and the FULL trk_last_error()
text of every case of the table below, and the early TRK_OK returns.  The entries share their back half (the unit lookup, the
nothing-to-test answer, the launch and the via sample count: coll_unit_for, nothing_to_test, launch_coll, via_samples in
csrc/trk_capi.hip); each keeps its own front half, and this file holds what a caller sees of it -- which check speaks first, and in
which words.

tests/golden/collision_entry_errors.json was recorded by running this same table (CASES) against the library built from the commit
BEFORE the entries were given their shared back half ("2-D point mass: one planning-loop body, one host path, one plan base"):
{case id: {"rc": code, "error": text, or null where the call returns TRK_OK}}.  Re-record with PYTHONPATH = the repository and tests/
(python tests/test_collision_entry_errors_cpu.py [path]) on UNCHANGED entries only.

Model, point set and cost model are blocks of zeros that are never dereferenced beyond their own fields: a zeroed model has 0 links,
0 DOF and its generated kernels disabled, a zeroed point set belongs to no model.  So the four via / point entries are stopped before
any device call even by a sound call ("generated kernels are disabled for this model", "belongs to no model"), and the table holds
sound calls for them.  trk_rollout_collision is not: a sound call with samples would go on to device work on BUF, which is no device
pointer -- every case of that entry carries a fault of its own or an empty batch (test_no_case_of_the_way_point_entry_reaches_the_device)."""
import ctypes as C
import json
import sys
from pathlib import Path

import pytest

from torch_robotics_amd import _abi, _lib

GOLDEN = Path(__file__).resolve().parent / "golden" / "collision_entry_errors.json"
NAN = float("nan")

MODEL, PS, CM = (C.c_char * 8192)(), (C.c_char * 8192)(), (C.c_char * 8192)()      # stand for TrkModel* / TrkPointSet* / TrkCostModel*
BUF = (C.c_float * 4096)()                                  # host memory standing for the device buffers, never read
BIG_H, BIG_N = 65537, 32768                                 # (horizon - 1) * n_interp = 2^31: beyond the limit


def coll(trk, m=MODEL, c=CM, fields=7, q=BUF, batch=2, horizon=8, margin=NAN, out=BUF, ws=BUF):
    """trk_rollout_collision"""
    return trk.trk_rollout_collision(m, c, fields, q, batch, horizon, margin, out, ws, None)


def via(trk, m=MODEL, c=CM, fields=7, x=BUF, batch=2, horizon=8, state_dim=7, n_interp=2, alpha=BUF, beta=BUF, margin=NAN, out=BUF):
    """trk_rollout_collision_via"""
    return trk.trk_rollout_collision_via(m, c, fields, x, batch, horizon, state_dim, n_interp, alpha, beta, margin, out, None)


def via_flags(trk, m=MODEL, c=CM, fields=7, x=BUF, batch=2, horizon=8, state_dim=7, n_interp=2, alpha=BUF, beta=BUF, margin=NAN,
              q_min=BUF, q_max=BUF, out=BUF, traj_flags=BUF):
    """trk_rollout_collision_via_flags"""
    return trk.trk_rollout_collision_via_flags(m, c, fields, x, batch, horizon, state_dim, n_interp, alpha, beta, margin, q_min, q_max,
                                               out, traj_flags, None)


def pcoll(trk, m=PS, c=CM, fields=7, q=BUF, batch=2, horizon=8, margin=NAN, out=BUF, ws=BUF):
    """trk_rollout_points_collision (m: the point set)"""
    return trk.trk_rollout_points_collision(m, c, fields, q, batch, horizon, margin, out, ws, None)


def pvia(trk, m=PS, c=CM, fields=7, x=BUF, batch=2, horizon=8, state_dim=7, n_interp=2, alpha=BUF, beta=BUF, margin=NAN,
         q_min=None, q_max=None, out=BUF, traj_flags=None):
    """trk_rollout_points_collision_via (m: the point set)"""
    return trk.trk_rollout_points_collision_via(m, c, fields, x, batch, horizon, state_dim, n_interp, alpha, beta, margin, q_min, q_max,
                                                out, traj_flags, None)


ENTRIES = (coll, via, via_flags, pcoll, pvia)
WAYPOINT, VIA, FLAGS = (coll, pcoll), (via, via_flags, pvia), (via_flags, pvia)


def _table():
    """[(case id, entry, keyword arguments that differ from a sound call)]"""
    t = []

    def add(entry, label, **kw):
        if entry is coll and not _own_fault(kw):
            kw, label = dict(kw, batch=0), label + " (batch = 0)"       # see the module docstring
        t.append((f"{entry.__name__}: {label}", entry, kw))

    # ---- each null argument
    for e in ENTRIES:
        for name in ("m", "c", "out"):
            add(e, f"null {name}", **{name: None})
    for e in WAYPOINT:
        add(e, "null q", q=None)
        add(e, "null ws", ws=None, batch=0)
    for e in VIA:
        for name in ("x", "alpha", "beta"):
            add(e, f"null {name}", **{name: None})
    for name in ("q_min", "q_max", "traj_flags"):
        add(via_flags, f"null {name}", **{name: None})
    # ---- masks
    for e in ENTRIES:
        for f in (0, 8, -1, 15, 1, 2, 3, 4, 5, 6, 7):
            add(e, f"fields = {f}", fields=f)
        # ---- sizes
        add(e, "batch = -1", batch=-1)
        for h in (-3, 0, 1, 2):
            add(e, f"horizon = {h}", horizon=h)
    for e in VIA:
        for n in (0, -1):
            add(e, f"n_interp = {n}", n_interp=n)
        add(e, "state_dim = 0", state_dim=0)
        add(e, "state_dim = -1", state_dim=-1)
        add(e, "(horizon - 1) * n_interp = 2^31", horizon=BIG_H, n_interp=BIG_N)
        add(e, "(horizon - 1) * n_interp = 2^31, batch = 0", horizon=BIG_H, n_interp=BIG_N, batch=0)
        add(e, "(horizon - 1) * n_interp = 2^31 - 65536: within the limit", horizon=BIG_H - 2, n_interp=BIG_N)
    # ---- every partial combination of traj_flags / q_min / q_max, and all three
    for e in FLAGS:
        for k in range(8):
            given = [n for b, n in ((1, "traj_flags"), (2, "q_min"), (4, "q_max")) if k & b]
            add(e, "given: " + (" + ".join(given) or "none of traj_flags / q_min / q_max"),
                **{n: (BUF if n in given else None) for n in ("traj_flags", "q_min", "q_max")})
    # ---- two faults at once: the order of the checks, every adjacent pair of each entry
    for e in (coll, via, via_flags):
        add(e, "null m + null c", m=None, c=None)
        add(e, "null c + batch = -1", c=None, batch=-1)
        add(e, "null c + horizon = 0", c=None, horizon=0)
    add(coll, "batch = -1 + fields = 0", batch=-1, fields=0)
    add(coll, "horizon = 0 + fields = 8", horizon=0, fields=8)
    add(coll, "fields = 0 + null q", fields=0, q=None)
    add(coll, "fields = 8 + null out", fields=8, out=None)
    add(coll, "null q + null out", q=None, out=None)
    add(coll, "null q + batch = 0", q=None, batch=0)
    for e in (via, via_flags):
        add(e, "horizon = 0 + n_interp = 0", horizon=0, n_interp=0)
        add(e, "batch = -1 + null alpha", batch=-1, alpha=None)
        add(e, "horizon = 1 + limit", horizon=1, n_interp=BIG_N)
        add(e, "fields = 0 + limit", fields=0, horizon=BIG_H, n_interp=BIG_N)
        add(e, "null beta + limit", beta=None, horizon=BIG_H, n_interp=BIG_N)
        add(e, "limit + null x", horizon=BIG_H, n_interp=BIG_N, x=None)
        add(e, "null x + null out", x=None, out=None)
        add(e, "null x + batch = 0", x=None, batch=0)
        add(e, "null out + batch = 0", out=None, batch=0)
    add(via_flags, "null traj_flags + null m", traj_flags=None, m=None)
    add(via_flags, "null q_min + fields = 0", q_min=None, fields=0)
    add(via_flags, "null q_max + limit", q_max=None, horizon=BIG_H, n_interp=BIG_N)
    add(via_flags, "null q_max + batch = 0", q_max=None, batch=0)
    for e in (pcoll, pvia):
        add(e, "null m + null c", m=None, c=None)
        add(e, "null c + fields = 0", c=None, fields=0)
        add(e, "fields = 8 + batch = -1", fields=8, batch=-1)
        add(e, "fields = 0 + horizon = 0", fields=0, horizon=0)
    add(pcoll, "batch = -1 + null q", batch=-1, q=None)
    add(pcoll, "horizon = 0 + null out", horizon=0, out=None)
    add(pcoll, "null q + no model", q=None)
    add(pcoll, "null q + batch = 0", q=None, batch=0)
    add(pvia, "horizon = 1 + n_interp = 0", horizon=1, n_interp=0)
    add(pvia, "batch = -1 + state_dim = 0", batch=-1, state_dim=0)
    add(pvia, "n_interp = 0 + only traj_flags", n_interp=0, traj_flags=BUF)
    add(pvia, "null alpha + only q_min", alpha=None, q_min=BUF)
    add(pvia, "only q_max + limit", q_max=BUF, horizon=BIG_H, n_interp=BIG_N)
    add(pvia, "limit + null x", horizon=BIG_H, n_interp=BIG_N, x=None)
    add(pvia, "null x + no model", x=None)
    add(pvia, "null out + no model", out=None)
    add(pvia, "null x + batch = 0", x=None, batch=0)
    # ---- the empty batch, with and without buffers
    for e in WAYPOINT:
        add(e, "batch = 0", batch=0)
        add(e, "batch = 0, null buffers", batch=0, q=None, out=None, ws=None)
    for e in VIA:
        add(e, "batch = 0", batch=0)
        add(e, "batch = 0, null buffers", batch=0, x=None, out=None)
    # ---- sound calls (not for trk_rollout_collision)
    for e in (via, via_flags, pcoll, pvia):
        add(e, "sound")
        add(e, "sound, margin 0.07", margin=0.07)
    add(pvia, "sound, with the flags", q_min=BUF, q_max=BUF, traj_flags=BUF)
    return t


def _own_fault(kw):
    """does a trk_rollout_collision call with these arguments end before its first device call?  (a null handle, a bad mask or size, a
    null q / out, an empty batch; a null scratch alone does not)"""
    return (any(kw.get(k, BUF) is None for k in ("m", "c", "q", "out")) or kw.get("fields", 7) not in range(1, 8) or
            kw.get("batch", 2) <= 0 or kw.get("horizon", 8) < 1)


CASES = _table()


def answer(trk, entry, kw):
    """what a caller sees of one call: the code, and the error text where there is one"""
    rc = entry(trk, **kw)
    return {"rc": rc, "error": None if rc == _abi.TRK_OK else trk.trk_last_error().decode("utf-8")}


def record(path=GOLDEN):
    """writes the file the test compares against: the same table, so the two cannot drift apart"""
    trk = _lib.lib()
    got = {cid: answer(trk, e, kw) for cid, e, kw in CASES}
    Path(path).write_text(json.dumps(got, indent=1, sort_keys=True) + "\n")
    return got


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
    assert codes == {_abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG, _abi.TRK_ERR_UNSUPPORTED}         # the table reaches every kind of answer
    assert all((v["error"] is None) == (v["rc"] == _abi.TRK_OK) for v in golden.values())


def test_no_case_of_the_way_point_entry_reaches_the_device(golden):
    mine = [(cid, kw) for cid, e, kw in CASES if e is coll]
    assert len(mine) > 30
    for cid, kw in mine:
        assert _own_fault(kw), cid
        assert golden[cid]["rc"] in (_abi.TRK_OK, _abi.TRK_ERR_INVALID_ARG), cid
        assert golden[cid]["rc"] != _abi.TRK_OK or kw["batch"] == 0, cid


@pytest.mark.parametrize("entry", ENTRIES, ids=lambda e: e.__name__)
def test_every_call_gets_the_recorded_code_and_text(trk, golden, entry):
    got = {cid: answer(trk, e, kw) for cid, e, kw in CASES if e is entry}
    assert len(got) > 30
    wrong = {cid: (g, golden[cid]) for cid, g in got.items() if g != golden[cid]}
    assert not wrong, wrong


def test_the_stops_before_the_device_are_the_recorded_ones(golden):
    """what keeps a sound call on zeroed handles from device work, per entry"""
    for e, text in ((via, "generated kernels are disabled for this model"), (via_flags, "generated kernels are disabled for this model"),
                    (pcoll, "the point set belongs to no model"), (pvia, "the point set belongs to no model")):
        for label in ("sound", "sound, margin 0.07"):
            assert golden[f"{e.__name__}: {label}"]["error"].endswith(text), (e.__name__, label)


if __name__ == "__main__":
    record(*sys.argv[1:2])
