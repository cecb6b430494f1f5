"""`Zoo`: one-line constructors of classical convex problems (reference: src/Zoo/*.jl, docs/src/zoo.md).

Each constructor takes a `MultiGrid` and returns an assembled `MGBProblem` built through `assemble` and the convex
constructors; solve it with `mgb_solve(problem, ...)`.  Problem parameters (`p`, forcing `f`, boundary data `g_u`, ...)
are keywords of the constructor, solver controls (`tol`, ...) keywords of `mgb_solve`.  Index lists are 1-based and
per-node matrices column-major, as in the reference.  Closed-form defaults are evaluated vectorised over the nodes;
a user callable is called once per node.

The vector-valued problems (`p_harmonic`, `norton_hoff`, 3-D `minimal_surface`) carry power cones wider than four
entries and up to 13 D rows; the device runs them on its wide path.  Phase I of a 3-D vector problem would need a
fifth state component, which this build does not have: give those problems a feasible start (the default `s_init`).
"""
from __future__ import annotations

from typing import Callable, Optional

import numpy as np

from .convex import convex_Euclidian_power, convex_linear, intersect
from .multigrid import MultiGrid
from .problem import MGBProblem, assemble, default_D, default_idx

__all__ = ["elastoplastic_torsion", "minimal_surface", "p_harmonic", "norton_hoff", "rof", "two_sided_obstacle"]

_OPS = ("dx", "dy", "dz")


def _dim(mg: MultiGrid) -> int:
    return int(mg.geometry.discretization.dim)


def _nodes(mg: MultiGrid) -> np.ndarray:
    return mg.geometry.xflat


def _per_node(fn: Callable, x: np.ndarray, width: int) -> np.ndarray:
    """One call of a user callable per node (as `convex._grid`); scalars and length-`width` sequences accepted."""
    out = np.empty((x.shape[0], width))
    for i, xi in enumerate(x):
        v = np.atleast_1d(np.asarray(fn(xi), dtype=np.float64)).reshape(-1)
        if v.size != width:
            raise ValueError(f"callable returned {v.size} value(s) per node, expected {width}")
        out[i] = v
    return out


def _scalar_grid(fn: Optional[Callable], default: np.ndarray, x: np.ndarray) -> np.ndarray:
    return default if fn is None else _per_node(fn, x, 1)[:, 0]


def _vector_state_setup(mg: MultiGrid, f: Optional[Callable], g_u: Optional[Callable], s_init: float,
                        f_default: np.ndarray, g_default: np.ndarray):
    """State (u_1, .., u_d, s); D = per component an id row and d partials, then s:id; f on the u_i:id rows and 1 on the
    slack row; idx = the y-positions of the d^2 partials and the slack (1-based).  reference: src/Zoo/Zoo.jl."""
    d = _dim(mg)
    x = _nodes(mg)
    n = x.shape[0]
    state_variables = [(f"u{i}", "dirichlet") for i in range(1, d + 1)] + [("s", "full")]
    D = []
    for i in range(1, d + 1):
        D.append((f"u{i}", "id"))
        D += [(f"u{i}", _OPS[j]) for j in range(d)]
    D.append(("s", "id"))
    nrows = len(D)                                   # d (1 + d) + 1
    fv = f_default if f is None else _per_node(f, x, d)
    gv = g_default if g_u is None else _per_node(g_u, x, d)
    f_grid = np.zeros((n, nrows))
    f_grid[:, [i * (d + 1) for i in range(d)]] = fv
    f_grid[:, nrows - 1] = 1.0
    g_grid = np.concatenate([gv, np.full((n, 1), float(s_init))], axis=1)
    idx = tuple((i - 1) * (d + 1) + 1 + j for i in range(1, d + 1) for j in range(1, d + 1)) + (nrows,)
    return state_variables, D, f_grid, g_grid, idx


def _scalar_fg(nrows: int, fv: np.ndarray, gv: np.ndarray, s_init: float):
    """f on the u:id row, 1/2 on the slack row; g = (g_u, s_init).  reference: src/Zoo/Zoo.jl `_scalar_fg`."""
    n = fv.shape[0]
    f_grid = np.zeros((n, nrows))
    f_grid[:, 0] = fv
    f_grid[:, nrows - 1] = 0.5
    g_grid = np.stack([gv, np.full(n, float(s_init))], axis=1)
    return f_grid, g_grid


def _const_grid(n: int, row) -> np.ndarray:
    return np.tile(np.asarray(row, dtype=np.float64).reshape(1, -1), (n, 1))


def elastoplastic_torsion(mg: MultiGrid, f: Optional[Callable] = None, g_u: Optional[Callable] = None, smax: float = 1.0,
                          s_init: Optional[float] = None) -> MGBProblem:
    """Hencky elasto-plastic torsion: min int |grad u|^2 / 2 + f u  s.t. |grad u| <= smax, as s >= |grad u|^2 and
    s <= smax^2.  Defaults: f = 2 / 4 / 16 in 1-D / 2-D / 3-D, g_u = 0, s_init = smax^2 / 2.
    reference: src/Zoo/elastoplastic_torsion.jl."""
    d = _dim(mg)
    x = _nodes(mg)
    n = x.shape[0]
    nrows = d + 2
    smax2 = float(smax) ** 2
    if s_init is None:
        s_init = smax2 / 2
    fv = _scalar_grid(f, np.full(n, 2.0 if d == 1 else 4.0 if d == 2 else 16.0), x)
    gv = _scalar_grid(g_u, np.zeros(n), x)
    f_grid, g_grid = _scalar_fg(nrows, fv, gv, s_init)
    Q_slack = convex_Euclidian_power(mg, idx=default_idx(d), p_grid=np.full(n, 2.0))
    Q_yield = convex_linear(mg, idx=(nrows,), A_grid=np.full((n, 1), -1.0), b_grid=np.full((n, 1), smax2))
    Q = intersect(mg, Q_slack, Q_yield)
    return assemble(mg, state_variables=[("u", "dirichlet"), ("s", "full")], D=default_D(d), f_grid=f_grid,
                    g_grid=g_grid, Q=Q)


def minimal_surface(mg: MultiGrid, g_u: Optional[Callable] = None, s_init: float = 10.0) -> MGBProblem:
    """Minimal surface in graph form: min int sqrt(1 + |grad u|^2), as s >= sqrt(|grad u|^2 + 1), the shifted Lorentz
    cone whose A y + b packs (grad u, 1, s).  Default g_u: x1^2 / 2 (1-D), (x1^2 - x2^2) / 2 (2-D), |x|^2 / 2 (3-D).
    reference: src/Zoo/minimal_surface.jl."""
    d = _dim(mg)
    x = _nodes(mg)
    n = x.shape[0]
    nrows = d + 2
    if g_u is None:
        gv = (0.5 * x[:, 0] ** 2 if d == 1 else 0.5 * (x[:, 0] ** 2 - x[:, 1] ** 2) if d == 2 else
              0.5 * np.sum(x[:, :d] ** 2, axis=1))
    else:
        gv = _per_node(g_u, x, 1)[:, 0]
    f_grid = np.zeros((n, nrows))
    f_grid[:, nrows - 1] = 1.0
    g_grid = np.stack([gv, np.full(n, float(s_init))], axis=1)
    nz = nrows
    A = np.zeros((nz, nz))
    for i in range(d):
        A[i, i + 1] = 1.0          # z[i] = du/dx_i = y[i + 1]
    A[nz - 1, nz - 1] = 1.0        # z[nz - 1] = s
    b = np.zeros(nz)
    b[d] = 1.0
    Q = convex_Euclidian_power(mg, idx=tuple(range(1, nz + 1)), A_grid=_const_grid(n, A.reshape(-1, order="F")),
                               b_grid=_const_grid(n, b), p_grid=np.ones(n))
    return assemble(mg, state_variables=[("u", "dirichlet"), ("s", "full")], D=default_D(d), f_grid=f_grid,
                    g_grid=g_grid, Q=Q)


def _vector_defaults(mg: MultiGrid, x: np.ndarray, first_1d=None):
    d = _dim(mg)
    n = x.shape[0]
    f_default = np.full((n, d), 0.5)
    g_default = np.zeros((n, d))
    g_default[:, 0] = first_1d(x) if (d == 1 and first_1d is not None) else np.prod(x[:, :d], axis=1)
    return f_default, g_default


def p_harmonic(mg: MultiGrid, p: float = 1.5, f: Optional[Callable] = None, g_u: Optional[Callable] = None,
               s_init: float = 100.0) -> MGBProblem:
    """Vectorial p-Laplacian: min int |grad u|_F^p + f . u for u: Omega -> R^d, slack s >= |grad u|_F^p.
    Defaults: f = (0.5, .., 0.5), g_u = (x1^2,) in 1-D and (x1 x2 (x3), 0, ..) otherwise.  reference: src/Zoo/p_harmonic.jl."""
    x = _nodes(mg)
    n = x.shape[0]
    f_default, g_default = _vector_defaults(mg, x, first_1d=lambda x: x[:, 0] ** 2)
    sv, D, f_grid, g_grid, idx = _vector_state_setup(mg, f, g_u, s_init, f_default, g_default)
    Q = convex_Euclidian_power(mg, idx=idx, p_grid=np.full(n, float(p)))
    return assemble(mg, state_variables=sv, D=D, f_grid=f_grid, g_grid=g_grid, Q=Q)


def _norton_hoff_A(d: int) -> np.ndarray:
    """A with A y[idx] = (eps_11 .. eps_dd, (du_i/dx_j + du_j/dx_i) / sqrt 2 for i < j, 0 .., s): |q|^2 = |eps(u)|_F^2."""
    nz = d * d + 1
    A = np.zeros((nz, nz))
    col = lambda i, j: i * d + j           # 0-based position of du_i/dx_j within y[idx]
    for r in range(d):
        A[r, col(r, r)] = 1.0
    row = d
    for i in range(d):
        for j in range(i + 1, d):
            A[row, col(i, j)] = A[row, col(j, i)] = 1.0 / np.sqrt(2.0)
            row += 1
    A[nz - 1, nz - 1] = 1.0
    return A


def norton_hoff(mg: MultiGrid, p: float = 1.5, f: Optional[Callable] = None, g_u: Optional[Callable] = None,
                s_init: float = 100.0) -> MGBProblem:
    """Norton-Hoff power-law elasticity: min int |eps(u)|_F^p + f . u with eps the symmetric gradient, in 2-D and 3-D
    (1-D raises).  Defaults: f = (0.5, .., 0.5), g_u = (x1 x2 (x3), 0, ..).  reference: src/Zoo/norton_hoff.jl."""
    d = _dim(mg)
    if d == 1:
        raise ValueError("norton_hoff: 1D not supported (symmetric gradient = scalar gradient; "
                         "use scalar p-Poisson or elastoplastic_torsion).")
    x = _nodes(mg)
    n = x.shape[0]
    f_default, g_default = _vector_defaults(mg, x)
    sv, D, f_grid, g_grid, idx = _vector_state_setup(mg, f, g_u, s_init, f_default, g_default)
    nz = len(idx)
    Q = convex_Euclidian_power(mg, idx=idx, A_grid=_const_grid(n, _norton_hoff_A(d).reshape(-1, order="F")),
                               b_grid=np.zeros((n, nz)), p_grid=np.full(n, float(p)))
    return assemble(mg, state_variables=sv, D=D, f_grid=f_grid, g_grid=g_grid, Q=Q)


def rof(mg: MultiGrid, f_data: Optional[Callable] = None, lam: float = 1.0, g_u: Optional[Callable] = None,
        s_init: float = 10.0, r_init: float = 10.0, **kw) -> MGBProblem:
    """Rudin-Osher-Fatemi denoising: min int |grad u| + lam/2 (u - f_data)^2, state (u, s, r) with s >= |grad u| and
    r >= (u - f_data)^2.  Defaults: f_data = tanh(5 x1) / 2, g_u = f_data.  `λ=` is accepted for `lam`.
    reference: src/Zoo/rof.jl."""
    if "λ" in kw:
        lam = kw.pop("λ")
    if kw:
        raise TypeError(f"rof: unexpected keyword(s) {sorted(kw)}")
    d = _dim(mg)
    x = _nodes(mg)
    n = x.shape[0]
    nrows = d + 3
    fd = 0.5 * np.tanh(5.0 * x[:, 0]) if f_data is None else _per_node(f_data, x, 1)[:, 0]
    gv = fd if g_u is None else _per_node(g_u, x, 1)[:, 0]
    D = [("u", "id")] + [("u", _OPS[j]) for j in range(d)] + [("s", "id"), ("r", "id")]
    f_grid = np.zeros((n, nrows))
    f_grid[:, nrows - 2] = 1.0
    f_grid[:, nrows - 1] = float(lam) / 2
    g_grid = np.stack([gv, np.full(n, float(s_init)), np.full(n, float(r_init))], axis=1)
    Q_tv = convex_Euclidian_power(mg, idx=tuple(range(2, d + 2)) + (nrows - 1,), p_grid=np.ones(n))
    Q_data = convex_Euclidian_power(mg, idx=(1, nrows), A_grid=_const_grid(n, [1.0, 0.0, 0.0, 1.0]),
                                    b_grid=np.stack([-fd, np.zeros(n)], axis=1), p_grid=np.full(n, 2.0))
    Q = intersect(mg, Q_tv, Q_data)
    return assemble(mg, state_variables=[("u", "dirichlet"), ("s", "full"), ("r", "full")], D=D, f_grid=f_grid,
                    g_grid=g_grid, Q=Q)


def two_sided_obstacle(mg: MultiGrid, f: Optional[Callable] = None, g_u: Optional[Callable] = None,
                       psi_lower: Optional[Callable] = None, psi_upper: Optional[Callable] = None,
                       s_init: float = 10.0, **kw) -> MGBProblem:
    """Membrane between two obstacles: min int |grad u|^2 / 2 + f u s.t. psi_lower <= u <= psi_upper.  Defaults:
    f = 1 / 2 / 8 in 1-D / 2-D / 3-D, g_u = 0, psi_lower = -0.1, psi_upper = 1.  `ψ_lower=` / `ψ_upper=` are accepted.
    reference: src/Zoo/two_sided_obstacle.jl."""
    psi_lower = kw.pop("ψ_lower", psi_lower)
    psi_upper = kw.pop("ψ_upper", psi_upper)
    if kw:
        raise TypeError(f"two_sided_obstacle: unexpected keyword(s) {sorted(kw)}")
    d = _dim(mg)
    x = _nodes(mg)
    n = x.shape[0]
    nrows = d + 2
    fv = _scalar_grid(f, np.full(n, 1.0 if d == 1 else 2.0 if d == 2 else 8.0), x)
    gv = _scalar_grid(g_u, np.zeros(n), x)
    f_grid, g_grid = _scalar_fg(nrows, fv, gv, s_init)
    lo = _scalar_grid(psi_lower, np.full(n, -0.1), x)
    hi = _scalar_grid(psi_upper, np.ones(n), x)
    Q_slack = convex_Euclidian_power(mg, idx=default_idx(d), p_grid=np.full(n, 2.0))
    Q_box = convex_linear(mg, idx=(1,), A_grid=_const_grid(n, [1.0, -1.0]), b_grid=np.stack([-lo, hi], axis=1))
    Q = intersect(mg, Q_slack, Q_box)
    return assemble(mg, state_variables=[("u", "dirichlet"), ("s", "full")], D=default_D(d), f_grid=f_grid,
                    g_grid=g_grid, Q=Q)
