"""The planted scenes of the new-map-point tests (tests/newpts_planted.py) on the CPU: the builder's guarantees at 16 cameras, and
oracle.new_map_points_from_pairs_c -- the C form that bench.py's CPU leg times -- against the Python restatement where tracks have 9
to 16 views."""
import numpy as np

from tests import newpts_planted as P


def test_builder_guarantees_at_16_cameras():
    """every planted track without a bad view becomes a point that holds exactly its views, every track with one becomes none; slot
    order is not track order; scores tie"""
    specs = P.every_c0_nv(16) + [dict(c0=c0, nv=nv, bad_view=(c0 + nv) % nv) for nv in (2, 3, 8, 9, 16) for c0 in range(0, 17 - nv, 3)]
    S = P.planted_scene(16, 250, 3, specs)              # (asserts the guarantees itself)
    res, o = P.run_restatement(S)
    pts = P.points_of(S, o, check=True)
    assert sum(m >= 0 for m in pts) == 120 == len(res["new"]) and sum(m < 0 for m in pts) == len(specs) - 120
    assert len(res["tracks"]) >= len(specs)             # (a rejected track is still a track)
    firsts = [views[0][1] for views in S["planted"] if views[0][0] == 0]
    assert firsts != sorted(firsts)
    scores = [q[3] for pl in S["pairs"] for q in pl]
    assert len(set(scores)) < len(scores) and all(0.8 <= v <= 1.0 for v in scores)
    assert all(len(pl) == len({q[0] for q in pl}) == len({q[1] for q in pl}) for pl in S["pairs"])


def _c_form_equals(S, **kw):
    res, o = P.run_restatement(S, **kw)
    res_c, o_c = P.run_restatement(S, c_form=True, **kw)
    assert res["new"] == res_c["new"] and res["map_count"] == res_c["map_count"] and np.array_equal(res["matches"], res_c["matches"])
    for k in ("mapPts", "mapCov", "flags", "newPt", "first", "pf"):
        assert np.array_equal(o[k], o_c[k]), k
    assert all(np.array_equal(o["s2m"][c], o_c["s2m"][c]) for c in range(S["nC"]))
    return res, o


def test_c_form_equals_the_restatement_on_every_c0_nv_at_16_cameras():
    res, _ = _c_form_equals(P.planted_scene(16, 250, 116, P.every_c0_nv(16)))
    assert len(res["new"]) == 120 and max(len(t) for t in res["tracks"]) == 16


def test_c_form_equals_the_restatement_on_the_second_register_set_scene():
    S = P.planted_scene(16, 250, 7, P.second_register_set_specs(16))
    res, o = _c_form_equals(S)
    assert {int(v) for v in o["flags"][res["new"]]} >= {0, 1}
    _c_form_equals(P.planted_scene(16, 250, 8, P.second_register_set_specs(16, two_view=True)), min_len=3)


def test_decide_edge_scene_holds_all_six_outcomes():
    S = P.decide_edge_scene()
    res, o = _c_form_equals(S)
    assert {c for c, _ in P.expected_types_hold(S, o)} == {"dyn", "i", "ii", "iii", "iv", "v", "vi"}
