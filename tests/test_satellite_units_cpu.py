"""CPU-only checks of the one table of satellite units (codegen.SATELLITES) and of what hangs on it: the build list and every file
it writes (tests/golden/spec_units_r15.json: the sha1 of all 26 units, the first pin of the three _padam units); which units
jit.specialize / specialize_points / load_satellite_units request, and when, told by a recorder in place of the compiler and of
dlopen; the idents of two run-time units as literals (a changed hash input would orphan every user's cache under a new name); and the
answers of has_matching_unit / has_matching_points_unit, recorded before the column kinds shared one body."""
import hashlib
import json
import types

import numpy as np
import pytest

import helpers as hp
from torch_robotics_amd import codegen, jit
from torch_robotics_amd.kinematics import URDF_DIR
from torch_robotics_amd.kinmodel import KinModel

IIWA7_IDENT = "jit_51c0c0f763a73ec7_dda58717"
STRETCHED_BOX_IDENT = "jitp_ba4561808d7a4550_09644d42e94f9c8f_28d56af5"
MAIN, MAIN_POINTS = "generate_link_kernel_source", "generate_points_rollout_source"
_real_cached_unit = jit._cached_unit


def test_every_generated_file_keeps_its_text(tmp_path):
    want = json.loads((hp.GOLD / "spec_units_r15.json").read_text())
    names = codegen.generate_sources(tmp_path)
    assert len(want) == 26 and names == list(want)
    for n in names:
        assert hashlib.sha1((tmp_path / n).read_bytes()).hexdigest() == want[n], n
    # the table's row order is the link order of the satellites, each kind's units contiguous behind the 14 main units
    assert list(codegen.SATELLITES) == ["vadam", "via", "padam", "coll"]
    assert [n.rsplit("_", 1)[1][:-len(".hip")] for n in names[14:]] == [s for s in codegen.SATELLITES for _ in range(3)]
    assert [(k.suffix, k.points, k.deferred) for k in codegen.SATELLITES.values()] == [
        ("vadam", False, True), ("via", False, False), ("padam", True, True), ("coll", True, False)]


# ----------------------------------------------------------------------------------------------------------------------
# run-time load: which (unit, source generator) is requested, and when
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def rec(monkeypatch, tmp_path):
    """jit with a recorder for compiler and dlopen, an empty process state and JIT_DIR = tmp_path.  Every source generator returns
    its own name, so rec.requests lists (unit, generator) in the order the cached-compile step was asked."""
    r = types.SimpleNamespace(requests=[], loaded=[], rtc=[], sources=[])

    def named(name):
        def generate(*a, **k):
            r.sources.append(name)
            return name
        return generate

    def cached(ident, source, verbose=False):
        r.requests.append((f"spec_{ident}", source()))
        return tmp_path / f"spec_{ident}.so"

    def load(so, name, main=True):
        assert so == tmp_path / f"spec_{name}.so" and main == (not name.endswith(tuple(f"_{s}" for s in codegen.SATELLITES)))
        r.loaded.append(name)
        jit._loaded[name] = so

    def rtc(kin, t, ident):
        r.rtc.append(ident)
        return "code object"

    monkeypatch.setattr(jit, "JIT_DIR", tmp_path)
    for state in ("_loaded", "_loaded_templates", "_pending"):
        monkeypatch.setattr(jit, state, {})
    monkeypatch.delenv("TRK_JIT_VIA_UNITS", raising=False)
    monkeypatch.setattr(jit, "hipcc_available", lambda: True)
    monkeypatch.setattr(jit, "_cached_unit", cached)
    monkeypatch.setattr(jit, "_load_unit", load)
    monkeypatch.setattr(jit, "_load_unit_rtc", rtc)
    monkeypatch.setattr(jit, "_load_points_unit_rtc", rtc)
    for g in (MAIN, MAIN_POINTS):
        monkeypatch.setattr(codegen, g, named(g))
    monkeypatch.setattr(codegen, "SATELLITES", {s: k._replace(source=named(k.source.__name__)) for s, k in codegen.SATELLITES.items()})
    return r


def iiwa7():
    kin = hp.model("iiwa7")
    return kin, dict(obj_links=[3, 5, 7], self_pairs=[(7, 1), (6, 2)], ee_link=kin.n_links - 1)


def stretched_box():
    """the point set of test_gpu_points_adam.test_run_time_unit_gets_the_planning_loop"""
    m, pl, po, spec = hp.grasp_panda_setup()
    po = (po * np.float32(1.25)).astype(np.float32)
    spec.clamp_fields = 7
    spec.validate()
    return m, pl, po, spec


def first_request_of_the_iiwa7_unit(rec):
    """specialize asks for the main unit and its via-point cost unit; the planning loop with the via-point term waits for the first
    request, which compiles it once; a robot served by other units asks for nothing
    (test_arm_traj_via_cpu.test_run_time_units_get_their_kernels_on_the_first_request runs this case)"""
    kin, tmpl = iiwa7()
    ident = jit.specialize(kin, **tmpl)
    assert ident == IIWA7_IDENT
    assert rec.requests == [(f"spec_{ident}", MAIN), (f"spec_{ident}_via", "generate_via_cost_source")]
    assert rec.loaded == [ident, f"{ident}_via"] and list(jit._pending) == [(ident, "vadam")] and not rec.rtc
    assert jit.specialize(kin, **tmpl) == ident and len(rec.requests) == 2          # a second call compiles nothing
    assert jit.load_satellite_units(hp.model("panda_arm_no_gripper"), "vadam") == [] and len(rec.requests) == 2
    assert jit.load_satellite_units(kin, "padam") == [] and len(rec.requests) == 2
    assert jit.load_satellite_units(kin, "vadam") == [ident]
    assert rec.requests[2:] == [(f"spec_{ident}_vadam", "generate_via_adam_source")] and rec.loaded[2:] == [f"{ident}_vadam"]
    assert jit.load_satellite_units(kin, "vadam") == [] and len(rec.requests) == 3 and not jit._pending
    return ident


def test_the_switch_leaves_the_main_unit_alone(rec, monkeypatch):
    monkeypatch.setenv("TRK_JIT_VIA_UNITS", "0")
    kin, tmpl = iiwa7()
    ident = jit.specialize(kin, **tmpl)
    assert rec.requests == [(f"spec_{ident}", MAIN)] and rec.loaded == [ident] and not jit._pending
    assert jit.load_satellite_units(kin, "vadam") == [] and len(rec.requests) == 1


def test_pipeline_units_and_big_robots_get_no_satellite(rec):
    kin, tmpl = iiwa7()
    ident = jit.specialize(kin, pipeline=True, **tmpl)
    assert ident == IIWA7_IDENT + "_p" and rec.requests == [(f"spec_{ident}", MAIN_POINTS)] and rec.loaded == [ident]
    dual, t = codegen.template_for("dual_panda")
    assert dual.n_dofs == 14
    big = jit.specialize(dual, t.obj_links, t.self_pairs, t.ee_link, ee2_link=t.ee2_link)
    assert rec.requests[1:] == [(f"spec_{big}", MAIN)] and rec.loaded[1:] == [big] and not jit._pending
    assert jit.load_satellite_units(dual, "vadam") == [] and len(rec.requests) == 2


def test_an_attached_point_unit_gets_its_boolean_unit_and_later_its_planning_loop(rec):
    m, pl, po, spec = stretched_box()
    ident = jit.specialize_points(m, pl, po, spec)
    assert ident == STRETCHED_BOX_IDENT
    assert rec.requests == [(f"spec_{ident}", MAIN_POINTS), (f"spec_{ident}_coll", "generate_points_collision_source")]
    assert rec.loaded == [ident, f"{ident}_coll"] and list(jit._pending) == [(ident, "padam")]
    assert jit.specialize_points(m, pl, po, spec) == ident and len(rec.requests) == 2
    assert jit.load_satellite_units(m, "vadam") == [] and len(rec.requests) == 2
    assert jit.load_satellite_units(m, "padam") == [ident]
    assert rec.requests[2:] == [(f"spec_{ident}_padam", "generate_points_adam_source")] and rec.loaded[2:] == [f"{ident}_padam"]
    assert jit.load_satellite_units(m, "padam") == [] and len(rec.requests) == 3 and not jit._pending


def test_a_point_set_above_eight_dof_never_gets_the_planning_loop(rec):
    kin, _ = codegen.template_for("dual_panda")
    L = kin.n_links
    spec = types.SimpleNamespace(n_links_in=L, obj_link_idx=[1, 2], self_link_idx=[], self_pairs=[], ee_link=-1, ee2_link=-1)
    ident = jit.specialize_points(kin, np.arange(L), np.zeros((L, 3), np.float32), spec)
    assert ident and kin.n_dofs > 8
    assert rec.requests == [(f"spec_{ident}", MAIN_POINTS), (f"spec_{ident}_coll", "generate_points_collision_source")]
    assert not jit._pending and jit.load_satellite_units(kin, "padam") == [] and len(rec.requests) == 2


def test_without_hipcc_the_code_object_carries_no_satellite(rec, monkeypatch):
    monkeypatch.setattr(jit, "hipcc_available", lambda: False)
    kin, tmpl = iiwa7()
    ident = jit.specialize(kin, **tmpl)
    m, pl, po, spec = stretched_box()
    pident = jit.specialize_points(m, pl, po, spec)
    assert rec.rtc == [ident, pident] and not rec.requests and not rec.loaded and not jit._pending
    assert set(jit._loaded) == set(jit._loaded_templates) == {ident, pident}
    assert jit.load_satellite_units(kin, "vadam") == [] and jit.load_satellite_units(m, "padam") == [] and not rec.requests


def test_a_cache_hit_generates_nothing(rec, monkeypatch, tmp_path):
    ident = first_request_of_the_iiwa7_unit(rec)
    units = [u for u, _ in rec.requests]
    assert units == [f"spec_{ident}", f"spec_{ident}_via", f"spec_{ident}_vadam"]
    for u in units:
        (tmp_path / f"{u}.so").write_bytes(b"")
        (tmp_path / f"{u}.stamp").write_text(jit._generator_stamp())
    for state in ("_loaded", "_loaded_templates", "_pending"):
        monkeypatch.setattr(jit, state, {})
    monkeypatch.setattr(jit, "_cached_unit", _real_cached_unit)
    del rec.sources[:], rec.loaded[:]
    kin, tmpl = iiwa7()
    assert jit.specialize(kin, **tmpl) == ident and jit.load_satellite_units(kin, "vadam") == [ident]
    assert rec.loaded == [ident, f"{ident}_via", f"{ident}_vadam"] and rec.sources == []
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"{u}{e}" for u in units for e in (".so", ".stamp"))


# ----------------------------------------------------------------------------------------------------------------------
# idents and matching
# ----------------------------------------------------------------------------------------------------------------------
def test_unit_idents_are_stable():
    kin, tmpl = iiwa7()
    assert jit.unit_ident(kin, codegen.CollisionTemplate(**tmpl)) == IIWA7_IDENT
    m, pl, po, spec = stretched_box()
    pt = jit._points_template_of(m, pl, po, spec)
    assert f"jitp_{codegen.model_hash(m):016x}_{codegen.points_hash(pt.point_link, pt.point_offset):016x}_{jit.template_hash(pt)}" == \
        STRETCHED_BOX_IDENT


def spec_of(t, n_cols, **change):
    """the cost model's view of a template (what jit._template_of / _points_template_of read)"""
    cols = sorted({c for p in t.self_pairs for c in p})
    d = dict(n_links_in=n_cols, obj_link_idx=list(t.obj_cols if isinstance(t, codegen.PointsTemplate) else t.obj_links),
             self_link_idx=cols, self_pairs=[(cols.index(a), cols.index(b)) for a, b in t.self_pairs], ee_link=t.ee_link,
             ee2_link=t.ee2_link)
    if getattr(t, "virtual", None):
        d.update(virtual_src=[r[:2] for r in t.virtual], virtual_w=[r[2:] for r in t.virtual])
    d.update(change)
    return types.SimpleNamespace(**d)


def last_pair_swapped(spec):
    spec.self_pairs = spec.self_pairs[:-1] + [spec.self_pairs[-1][::-1]]
    return spec


# what the parent of the change that merged the two bodies answered: every bundled (robot, template) and point set is served, with
# or without an EE term; another obj list, another pair, an EE link that is not baked, or another point set is not
MISMATCHES = {"obj": False, "pair": False, "ee": False}


def test_matching_answers_as_before(monkeypatch):
    monkeypatch.setattr(jit, "_loaded_templates", {})
    for ident in codegen.SPEC_ROBOTS:
        kin, t = codegen.template_for(ident)
        assert jit.has_matching_unit(kin, spec_of(t, kin.n_links)) is True, ident
        assert jit.has_matching_unit(kin, spec_of(t, kin.n_links, ee_link=-1)) is True, ident
    kin, t = codegen.template_for("panda")
    got = {"obj": jit.has_matching_unit(kin, spec_of(t, kin.n_links, obj_link_idx=t.obj_links[:-1])),
           "pair": jit.has_matching_unit(kin, last_pair_swapped(spec_of(t, kin.n_links))),
           "ee": jit.has_matching_unit(kin, spec_of(t, kin.n_links, ee_link=t.ee_link - 1))}
    assert got == MISMATCHES
    assert not jit.has_matching_points_unit(kin, np.arange(kin.n_links), np.zeros((kin.n_links, 3), np.float32), spec_of(t, kin.n_links))
    for ident, (urdf, fn) in codegen.SPEC_POINT_ROBOTS.items():
        kin = KinModel.from_urdf(str(URDF_DIR / urdf))
        t = fn(kin)
        pl, po, P = t.point_link, t.point_offset, len(t.point_link)
        assert jit.has_matching_points_unit(kin, pl, po, spec_of(t, P)) is True, ident
        assert jit.has_matching_points_unit(kin, pl, po, spec_of(t, P, ee_link=-1)) is True, ident
        assert jit.has_matching_points_unit(kin, pl, po * np.float32(1.25), spec_of(t, P)) is False, ident
        got = {"obj": jit.has_matching_points_unit(kin, pl, po, spec_of(t, P, obj_link_idx=t.obj_cols[:-1])),
               "pair": jit.has_matching_points_unit(kin, pl, po, last_pair_swapped(spec_of(t, P))),
               "ee": jit.has_matching_points_unit(kin, pl, po, spec_of(t, P, ee_link=t.ee_link - 1))}
        assert got == MISMATCHES, ident


def test_matching_parses_the_bundled_point_robots_once(monkeypatch):
    monkeypatch.setattr(codegen, "_template_cache", {})
    calls = []
    real = KinModel.from_urdf.__func__
    monkeypatch.setattr(KinModel, "from_urdf", classmethod(lambda cls, *a, **k: calls.append(a) or real(cls, *a, **k)))
    m, pl, po, spec = stretched_box()
    del calls[:]
    assert not jit.has_matching_points_unit(m, pl, po, spec) and not jit.has_matching_points_unit(m, pl, po, spec)
    assert 0 < len(calls) <= len(codegen.SPEC_POINT_ROBOTS)
