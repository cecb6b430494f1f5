"""Curved (isoparametric) fem2d_P2 on the host: the `curved` opt-in, subdivision that keeps curved elements curved, the
dispatch of `interpolate._plan`, and the refusal of the ray casters.  No GPU: the device side is tests/test_gpu_curved_p2.py.
"""
import numpy as np
import pytest

import mgb_amd as m
from curved_p2_cases import LD, MESHES, manufactured, mesh_a, mesh_b, newton
from mgb_amd import fem2d_p2
from mgb_amd.contour import _contour_plan, default_refine
from mgb_amd.interpolate import P2, P2C, _plan
from mgb_amd.raycast import RayCaster, _raycast_plan, clip_box, render_volume

BUBBLES = [True, False]


def _same_arrays(g0, g1):
    return (np.array_equal(g0.x, g1.x) and np.array_equal(g0.t, g1.t) and np.array_equal(g0.w, g1.w)
            and all(np.array_equal(g0.operators[k].to_sparse().toarray(), g1.operators[k].to_sparse().toarray())
                    for k in ("id", "dx", "dy")))


# ---------------------------------------------------------------------------------------------------------------------
# 1. the flag
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bubble", BUBBLES)
def test_flag_defaults_to_false_is_carried_and_changes_no_array(bubble):
    assert m.fem2d_P2(bubble=bubble).discretization.curved is False
    assert m.subdivide(m.fem2d_P2(bubble=bubble), 2).discretization.curved is False
    assert fem2d_p2.geometric_mg(m.fem2d_P2(bubble=bubble), 2).geometry.discretization.curved is False
    for make in (mesh_a, mesh_b):
        g0, g1 = make(bubble, curved=False), make(bubble, curved=True)
        assert g0.discretization.curved is False and g1.discretization.curved is True
        assert _same_arrays(g0, g1)
        assert m.subdivide(g1, 2).discretization.curved is True
        assert fem2d_p2.geometric_mg(g1, 2).geometry.discretization.curved is True
        assert m.amg(g1).geometry.discretization.curved is True
        assert m.subdivide(g0, 2).discretization.curved is False
    s0, s1 = m.subdivide(m.fem2d_P2(bubble=bubble), 3), m.subdivide(m.fem2d_P2(bubble=bubble, curved=True), 3)
    assert s1.discretization.curved is True and _same_arrays(s0, s1)           # straight input: today's bits


# ---------------------------------------------------------------------------------------------------------------------
# 2., 3. subdivide keeps curved elements curved
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("curved", [False, True])
@pytest.mark.parametrize("bubble", BUBBLES)
@pytest.mark.parametrize("L", [1, 2, 3])
def test_subdivide_is_the_geometry_of_geometric_mg(L, bubble, curved):
    g = mesh_a(bubble, curved=curved)
    s, r = m.subdivide(g, L), fem2d_p2.geometric_mg(g, L).geometry
    assert s.x.shape == (g.x.shape[0], g.x.shape[1] * 4 ** (L - 1), 2)
    assert np.array_equal(s.x, r.x) and np.array_equal(s.t, r.t) and np.array_equal(s.w, r.w)
    assert s.discretization.curved is curved


@pytest.mark.parametrize("bubble", BUBBLES)
def test_subdivide_keeps_the_area(bubble):
    g = mesh_a(bubble)
    a0, a1 = float(np.sum(g.w)), float(np.sum(m.subdivide(g, 3).w))
    print(f"curved fem2d_P2 bubble={bubble}: sum(w) {a0!r} -> {a1!r}, relative change {abs(a1 - a0) / a0:.2e}")
    assert abs(a1 - a0) <= 1e-13 * a0


# ---------------------------------------------------------------------------------------------------------------------
# 4., 5. the dispatch of _plan
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bubble", BUBBLES)
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_plan_takes_the_curved_family_only_where_needed(mesh, bubble):
    g = MESHES[mesh](bubble)
    family, name, d, k, p, N, xnodes, table = _plan(g)
    assert family == P2C == 7 and name == "fem2d_P2" and (d, k, p, N) == (2, 2, 7 if bubble else 6, g.x.shape[1])
    assert np.array_equal(table, fem2d_p2.basis_coefficient_table(bubble)) and np.array_equal(xnodes, g.xflat)
    # a straight geometry takes today's path whatever the flag says
    for straight in (m.fem2d_P2(bubble=bubble, curved=True), m.subdivide(m.fem2d_P2(bubble=bubble, curved=True), 3)):
        assert _plan(straight)[0] == P2
    # without the flag the refusal is today's, with a hint appended
    with pytest.raises(ValueError, match=r"^fem2d_P2 interpolation needs straight elements: .* curved=True"):
        _plan(MESHES[mesh](bubble, curved=False))


def test_contour_and_stream_plans_accept_the_curved_family():
    g = mesh_a(True)
    assert _contour_plan(g)[0] == P2C and _contour_plan(g, "tessellate", surfaces_only=True)[0] == P2C
    assert default_refine(P2C, 2) == default_refine(P2, 2) == 2
    assert _raycast_plan(g, "StreamTracer", curved_p2=True)[0] == P2C


# ---------------------------------------------------------------------------------------------------------------------
# 6. the ray casters refuse curved P2 by name, before any device work
# ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    """Any attempt to load the library or open a device context fails the test (the pattern of tests/test_raycast.py)."""
    from mgb_amd import device

    def boom(*a, **k):
        raise AssertionError("the library was touched")
    monkeypatch.setattr(device, "load_library", boom)
    monkeypatch.setattr(device, "HipContext", boom)


@pytest.mark.parametrize("bubble", BUBBLES)
def test_ray_casters_refuse_curved_p2_by_name(no_library, bubble):
    g = mesh_a(bubble)
    with pytest.raises(ValueError, match=r"^RayCaster: curved fem2d_P2 geometries are not supported$"):
        RayCaster(g, np.zeros((1, 2)), np.ones((1, 2)), 0.1)
    with pytest.raises(ValueError, match=r"^clip_box: curved fem2d_P2 geometries are not supported$"):
        clip_box(g)
    with pytest.raises(ValueError, match=r"^render_volume: curved fem2d_P2 geometries are not supported$"):
        render_volume(g, np.zeros(g.xflat.shape[0]), (3.0, 2.0, 1.0), (0, 0, 0))
    # the straight geometry with the flag is cast as before
    assert np.array_equal(clip_box(m.fem2d_P2(bubble=bubble, curved=True)), clip_box(m.fem2d_P2(bubble=bubble)))


# ---------------------------------------------------------------------------------------------------------------------
# the host twin of the device's Newton iteration (the yardstick of the GPU tests) on its own
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bubble", BUBBLES)
@pytest.mark.parametrize("mesh", sorted(MESHES))
def test_the_float64_twin_converges_at_every_manufactured_point(mesh, bubble):
    g = MESHES[mesh](bubble)
    elem, made, pts = manufactured(g, np.random.default_rng(7), 20_000)
    l, its, ok, tol = newton(g, elem, pts, np.float64)
    err = np.abs(l - made).max(axis=1)
    print(f"curved fem2d_P2 twin mesh {mesh} bubble={bubble}: at most {its.max()} iterations, max |l - made| {err.max():.2e}, "
          f"stopping tolerance {tol.min():.2e} .. {tol.max():.2e}")
    assert ok.all() and its.max() <= 5
    # the step that met the stopping test was <= tol and Newton's next error is far below its last step; the rounding
    # of the point itself moves l by eps / 2 max|x| |J^{-1}|, which is tol / 128 at most
    assert np.all(err <= tol)
    lo = newton(g, elem, pts, LD, start=made)[0]
    assert np.all(np.abs(lo - made).max(axis=1) <= tol)                        # the oracle returns to where the point was made
