"""Hand-built fem1d hierarchies that put every shape-gated transfer, reduction and assembly kernel on both sides of its gate
(csrc/problem.cpp: upload_csr; csrc/assembly_plan.cpp: the assembly-plan gates; DESIGN.md "Shape gates"), with exact
references.

Every hierarchy is fem1d, k = 1, a uniform mesh of N elements (n = 2 N broken nodes), default D / f / g, the power cone with
p = 1.5, written out as plain dataclasses like helpers.literal_fem1d_problem.  The last level is the true finest one (interior
vertices for u, broken slack: selection rows); the coarser levels are synthetic CSR matrices R = blockdiag(U, S) whose row and
column lengths are chosen from the gates.  Next to every level stands the plan it must get (DeviceProblem.level_plan);
tests/test_gate_cases.py checks these literals against `restated_plan`, a Python restatement of the gate arithmetic from R
alone, and tests/test_gpu_gates.py against the device.

No projection kernel is out of reach of fem1d (p = 2 nodes per element): `accumulate`, `staged` and `mfma` are selected by
shape, the loop kernel `panel_project` by the same level as `mfma` under MGBHIP_NO_MFMA_PROJECT=1 (proj_wide, level m385), so
no fem2d_P2 / fem3d case is needed.

References.  All sums are exact rational arithmetic (`exact_sum`: the Fraction sum of exactly formed products, carried on the
common power-of-two denominator) and rounded once:
  prolongation  z + R s              per row i:   bound (len_i + 1) 2^-53 (|z_i| + sum_j |R_ij s_j|)
  restriction   R' ret               per entry j: bound ((len_j + 2) 2^-53 + KERNEL_RTOL) sum_i |R_ij ret_i|
  assembly      R' H_blk R           per entry:   the same two-term bound, len = the entry's contribution-list length
`ret` and `H_blk` are the oracle's fp64 fine gradient and broken-basis Hessian.  An entry is checked only if its smallest
non-zero term is >= SENSITIVITY x its bound (a dropped or doubled term is then a violation by that factor); at most
MAX_SKIPPED of the entries of a case may fail that."""
import functools
import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import scipy.sparse as sp

KERNEL_RTOL = 1e-10          # the project's per-kernel bar for device-versus-oracle (tests/test_gpu_parity.py)
U53 = 2.0 ** -53
SENSITIVITY = 64
MAX_SKIPPED = 0.05
SAMPLE = 512                 # entries checked on levels with m > ALL_BELOW (seeded; longest, shortest and empty always included)
ALL_BELOW = 385
CHUNK = 4096                 # csrc/kernels.hip: rows of R' per (row, chunk) workgroup
P_CONE = 1.5


# ---------------------------------------------------------------------------------------------------------------------
# the fem1d problem around a list of synthetic levels
# ---------------------------------------------------------------------------------------------------------------------

def fine_U(N):
    """u at the 2 N broken nodes from the N - 1 interior vertices (Dirichlet ends masked): selection rows."""
    v = np.arange(1, N)
    rows = np.concatenate([2 * v - 1, 2 * v])
    return sp.csr_matrix((np.ones(rows.size), (rows, np.concatenate([v - 1, v - 1]))), shape=(2 * N, N - 1))


def fem1d_problem(N, coarse, p=P_CONE):
    """helpers.literal_fem1d_problem for N uniform elements; `coarse`: [(U, S)] with U (2N x cu) and S (2N x cs) in CSR."""
    from mgb_amd.blockmatrices import BlockColumn, BlockDiag
    from mgb_amd.convex import KIND_EP, Convex, Piece
    from mgb_amd.multigrid import AMG, Geometry
    from mgb_amd.problem import MGBProblem
    nodes = np.linspace(-1.0, 1.0, N + 1)
    h = np.diff(nodes)
    n = 2 * N
    x = np.stack([nodes[:-1], nodes[1:]], axis=1).reshape(-1)                 # broken nodes, element-major
    w = np.repeat(h / 2, 2)
    ident = np.zeros((2, 2, N))
    ident[0, 0, :] = ident[1, 1, :] = 1.0
    dx = np.zeros((2, 2, N))
    dx[:, 0, :] = -1.0 / h
    dx[:, 1, :] = 1.0 / h
    ops = {"id": BlockDiag(ident), "dx": BlockDiag(dx)}
    geom = Geometry(discretization=None, t=np.stack([np.arange(N), np.arange(N) + 1]), x=x.reshape(N, 2, 1).transpose(1, 0, 2).copy(),
                    w=w, operators=ops)
    pairs = list(coarse) + [(fine_U(N), sp.identity(n, format="csr"))]
    D_spec = [(0, "id"), (0, "dx"), (1, "id")]
    main = AMG(geometry=geom, x=x.reshape(n, 1), w=w, R_fine=[sp.block_diag([U, S], format="csr") for U, S in pairs],
               D_fine=[BlockColumn(ops[name], state, 2) for (state, name) in D_spec], state_names=["u", "s"], D_spec=D_spec)
    D_spec2 = D_spec + [(2, "id"), (0, "id"), (1, "id")]
    feas = AMG(geometry=geom, x=x.reshape(n, 1), w=w, R_fine=[sp.block_diag([U, S, S], format="csr") for U, S in pairs],
               D_fine=[BlockColumn(ops[name], state, 3) for (state, name) in D_spec2],
               state_names=["u", "s", "feasibility_slack"], D_spec=D_spec2)
    Q = Convex([Piece(KIND_EP, (1, 2), np.tile([1.0, 0.0, 0.0, 1.0], (n, 1)), np.zeros((n, 2)), np.full(n, float(p)),
                      np.full(n, 1.0 if p < 2 else 2.0))])
    f = np.tile([0.5, 0.0, 1.0], (n, 1))
    g = np.stack([x, np.full(n, 2.0)], axis=1)
    return MGBProblem((main, feas), f, g, Q, geom)


def weight(i, j=0):
    """Smooth positive weights in [0.3, 0.95], never 1.0 and not all equal."""
    return 0.3 + 0.65 * np.cos(0.013 * np.asarray(i, dtype=np.float64) + 0.31 * np.asarray(j, dtype=np.float64)) ** 2


def hats(N, cu):
    """u: the cu interior P1 hat functions of a uniform coarse grid, sampled at the fine vertices (partition of unity)."""
    H = 2.0 / (cu + 1)
    rows, cols, vals = [], [], []
    nodes = np.linspace(-1.0, 1.0, N + 1)
    v = np.repeat(np.arange(N), 2) + np.tile([0, 1], N)                       # vertex of every broken node
    for k in range(cu):
        phi = 1.0 - np.abs(nodes[v] - (-1.0 + (k + 1) * H)) / H
        keep = np.flatnonzero((phi > 1e-9) & (v > 0) & (v < N))
        rows.append(keep); cols.append(np.full(keep.size, k)); vals.append(phi[keep])
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(2 * N, cu))


def aggregates(n, lengths):
    """S: column j covers the next lengths[j] consecutive broken nodes with smooth weights; nodes left over have empty rows."""
    assert sum(lengths) <= n
    rows = np.arange(sum(lengths))
    cols = np.repeat(np.arange(len(lengths)), lengths)
    return sp.csr_matrix((weight(rows), (rows, cols)), shape=(n, len(lengths)))


def spread(nodes, ncols):
    """ncols column lengths that cover `nodes` consecutive nodes as evenly as possible."""
    q, r = divmod(nodes, ncols)
    return [q + 1] * r + [q] * (ncols - r)


def windows(n, cs, width, groups=None):
    """S with dense rows: node i carries `width` consecutive columns starting at a window that slides from 0 to cs - width
    (partition-of-unity style: positive, normalised per row, not equal).  groups = (per_group, elements): element e uses the
    window of group e mod (cs // per_group) instead and elements >= `elements` keep empty rows."""
    rows, cols, vals = [], [], []
    for i in range(n):
        if groups is None:
            start = (i * (cs - width)) // max(n - 1, 1)
        else:
            e = i // 2
            if e >= groups[1]:
                continue
            start = (e % (cs // groups[0])) * groups[0]
        j = np.arange(start, start + width)
        v = weight(7 * i, j)
        rows.append(np.full(width, i)); cols.append(j); vals.append(v / v.sum() * (0.5 + 0.4 * math.sin(0.3 * i) ** 2) * width ** 0.5)
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, cs))


def row_groups(n, cs, wide):
    """S for the row-length gate: nodes [0, n/6): one entry (value != 1); [n/6, n/2): `wide` entries; [n/2, 2n/3): none;
    [2n/3, 3n/4): 64 entries; the rest one entry."""
    rows, cols, vals = [], [], []
    for i in range(n):
        if n // 6 <= i < n // 2:
            j = np.arange(wide)
        elif n // 2 <= i < 2 * n // 3:
            continue
        elif 2 * n // 3 <= i < 3 * n // 4:
            j = np.arange(64)
        else:
            j = np.array([i % cs])
        v = weight(5 * i, j)
        rows.append(np.full(j.size, i)); cols.append(j); vals.append(v / v.sum() if j.size > 1 else v)
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, cs))


def ranges_U(N, ranges):
    """u columns over element ranges [a, b) (both broken nodes of each element): synthetic, not Dirichlet.  The weights are a
    smooth function of the node's coordinate, so that u' stays O(1e-3) away from 1 on every mesh."""
    rows, cols = [], []
    for k, (a, b) in enumerate(ranges):
        r = np.arange(2 * a, 2 * b)
        rows.append(r); cols.append(np.full(r.size, k))
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    xi = ((rows + 1) // 2) / N                                                # vertex coordinate in [0, 1]
    return sp.csr_matrix((weight(200.0 * xi, cols), (rows, cols)), shape=(2 * N, len(ranges)))


# ---------------------------------------------------------------------------------------------------------------------
# the cases.  expect: the fields of DeviceProblem.level_plan that the level must show; assembly fields (selection ... mean_list)
# are listed where the level is assembled (ops contains "assemble"), since the plan is built by the first f2.
# ---------------------------------------------------------------------------------------------------------------------

@dataclass
class Level:
    name: str
    build: object                      # N -> (U, S)
    expect: dict
    ops: tuple = ("prolong", "restrict")
    switches: tuple = ()               # ((env name, expected projection under it), ...): assembled again in a worker process


@dataclass
class Case:
    name: str
    N: int
    levels: list
    finest: Level = None

    def all_levels(self):
        return self.levels + [self.finest]


def _finest(N, ops=("prolong", "restrict")):
    exp = dict(R_unit=True, R_long=False, T_long=False, T_chunks=0, max_row=1, max_col=2)
    if "assemble" in ops:
        exp.update(selection=True, acc=False, long_lists=False, gather_nchunk=0, projection="none")
    return Level("finest", None, exp, ops)


def _gen(R_long=False, T_long=False, T_chunks=0, **kw):
    return dict(R_unit=False, R_long=R_long, T_long=T_long, T_chunks=T_chunks, **kw)


def _asm(acc, projection, long_lists=False, gather_chunk=0, gather_nchunk=0, **kw):
    return dict(selection=False, acc=acc, long_lists=long_lists, gather_chunk=gather_chunk, gather_nchunk=gather_nchunk,
                projection=projection, **kw)


NA = 9300          # restrict_cols: 18 600 broken nodes
CU_A = 999         # hat supports of ~37 broken nodes: the u columns stay below every column-length gate


def _cols(lengths):
    return lambda N: (hats(N, CU_A), aggregates(2 * N, lengths))


CASES = [
    # -- column length of R: the restriction R' v.  Thread per row (<= 64) / wave per row (T_long) / (row, chunk) workgroups of
    #    CHUNK = 4096 entries plus a fixed-order sum (>= 1024 and R.cols <= 16384).  Every level also has a column with one entry
    #    and an empty one; its slack rows have one entry != 1 or none, so prolongation is the general row kernel.
    Case("restrict_cols", NA, [
        Level("mixed", _cols([64, 65, 1023, 1024, 4096, 4097, 2 * 4096 + 1, 1, 0]), _gen(T_long=True, T_chunks=3, max_row=2, max_col=8193)),
        Level("max64", _cols([64] * 20 + [1, 0]), _gen(T_long=False, max_row=2, max_col=64)),
        Level("max65", _cols([65, 64, 1, 0]), _gen(T_long=True, max_row=2, max_col=65)),
        Level("max1023", _cols([1023, 64, 1, 0]), _gen(T_long=True, max_row=2, max_col=1023)),
        Level("max1024", _cols([1024, 1023, 1, 0]), _gen(T_long=True, T_chunks=1, max_row=2, max_col=1024)),
        Level("max4096", _cols([4096, 1, 0]), _gen(T_long=True, T_chunks=1, max_row=2, max_col=4096)),
        Level("max4097", _cols([4097, 1, 0]), _gen(T_long=True, T_chunks=2, max_row=2, max_col=4097)),
        # R.cols = 16384 chunks its 1024-entry column, R.cols = 16385 must not
        Level("cols16384", _cols([1024, 0] + spread(2 * NA - 1024, 16384 - CU_A - 2)), _gen(T_long=True, T_chunks=1, max_row=2, max_col=1024)),
        Level("cols16385", _cols([1024, 0] + spread(2 * NA - 1024, 16385 - CU_A - 2)), _gen(T_long=True, T_chunks=0, max_row=2, max_col=1024)),
    ], _finest(NA)),
    # -- row length of R: the prolongation z0 + R s.  rows64: longest row 64 (prolong_kernel); rows65: 65 (R_long, wave per
    #    row); both have rows with one entry != 1 and rows with none.  m = 79 / 80 with wide supports: LDS accumulation.
    Case("prolong_rows", 300, [
        Level("rows64", lambda N: (hats(N, 15), row_groups(2 * N, 64, 64)), _gen(R_long=False, T_long=True, max_row=64, max_col=255)),
        Level("rows65", lambda N: (hats(N, 15), row_groups(2 * N, 65, 65)),
              _gen(R_long=True, T_long=True, max_row=65, max_col=255, **_asm(True, "accumulate", acc_split=1, cmax=65, mean_list=0)),
              ops=("prolong", "restrict", "assemble")),
    ], _finest(300)),
    # -- projection R' H_blk R on small levels, N = 64.  m2: acc (slab_est 256 >= 16 mt = 48).  m16: slab_est < 16 mt = 2176,
    #    no acc, narrow supports: staged.  m17: dense slack rows, slab_est >= 16 mt = 2448: acc.  finest: selection gather.
    Case("proj_small", 64, [
        Level("m2", lambda N: (hats(N, 1), aggregates(2 * N, [2 * N])),
              _gen(T_long=True, max_row=1, max_col=128, **_asm(True, "accumulate", acc_split=1, cmax=1, mean_list=0)),
              ops=("prolong", "restrict", "assemble")),
        Level("m16", lambda N: (hats(N, 8), aggregates(2 * N, [16] * 8)),
              _gen(T_long=False, max_row=2, max_col=28, **_asm(False, "staged", cmax=3, mean_list=6)),
              ops=("prolong", "restrict", "assemble")),
        Level("m17", lambda N: (hats(N, 8), windows(2 * N, 9, 9)),
              _gen(T_long=True, max_row=9, max_col=128, **_asm(True, "accumulate", acc_split=1, cmax=9, mean_list=0)),
              ops=("prolong", "restrict", "assemble")),
    ], _finest(64, ops=("prolong", "restrict", "assemble"))),
    # -- projection with wide supports, N = 8.  m = 384 and 385 both miss acc: at m = 384 the packed triangle (73 920 doubles)
    #    needs nsplit = 5 > 4 chunks of the 144 KiB LDS budget, so `nsplit <= 4` binds before `m <= 384` ever can.
    #    m384: about 50 columns per element, matrix cores; under MGBHIP_NO_MFMA_PROJECT the staged kernel.
    #    m385: ct = 196, matrix cores; under the switch the staging of 44 KiB exceeds 40 KiB: the loop kernel panel_project.
    Case("proj_wide", 8, [
        Level("m384", lambda N: (fine_U(N), windows(2 * N, 377, 24)),
              _gen(T_long=False, max_row=24, max_col=2, **_asm(False, "mfma", cmax=48, mean_list=1)),
              ops=("prolong", "restrict", "assemble"), switches=(("MGBHIP_NO_MFMA_PROJECT", "staged"), ("MGBHIP_NO_SORTED_SLAB", "mfma"))),
        Level("m385", lambda N: (fine_U(N), windows(2 * N, 378, 180)),
              _gen(R_long=True, T_long=False, max_row=180, max_col=14, **_asm(False, "mfma", cmax=194, mean_list=2)),
              ops=("prolong", "restrict", "assemble"), switches=(("MGBHIP_NO_MFMA_PROJECT", "loop"), ("MGBHIP_NO_SORTED_SLAB", "mfma"))),
    ], _finest(8)),
    # -- gather of contribution lists around mean length 48, N = 783, m = 385 (no acc): one u column over every element, slack
    #    in 16 groups of 24 columns, element e dense in group e mod 16: 9 985 structural entries.  mean49: 783 elements,
    #    489 375 summands, mean 49 > 48: wave per list.  mean48: 767 elements, 479 375 summands, mean 48: thread per list.
    Case("gather_mean", 783, [
        Level("mean49", lambda N: (ranges_U(N, [(0, N)]), windows(2 * N, 384, 24, groups=(24, N))),
              _gen(T_long=True, T_chunks=1, max_row=24, max_col=1566, **_asm(False, "mfma", long_lists=True, cmax=24, mean_list=49)),
              ops=("restrict", "assemble")),
        Level("mean48", lambda N: (ranges_U(N, [(0, 767)]), windows(2 * N, 384, 24, groups=(24, 767))),
              _gen(T_long=True, T_chunks=1, max_row=24, max_col=1534, **_asm(False, "mfma", long_lists=False, cmax=24, mean_list=48)),
              ops=("restrict", "assemble")),
    ], _finest(783, ops=())),
    # -- two-stage gather, N = 65 600 > 65 536 elements (no acc), m = 4: slack column over every node, three u columns over
    #    16 401, 16 399 and 16 400 elements.  maxlen = 65 600 = 64 x 1025 (an exact multiple of gather_chunk = 1025); the u
    #    lists are 16 x 1025 + 1, - 1 and + 0 long.  The restriction of the slack column runs in 33 chunks of 4096.
    Case("gather_two_stage", 65600, [
        Level("m4", lambda N: (ranges_U(N, [(0, 16401), (16401, 32800), (32800, 49200)]), aggregates(2 * N, [2 * N])),
              _gen(T_long=True, T_chunks=33, max_row=1, max_col=131200,
                   **_asm(False, "staged", long_lists=True, gather_chunk=1025, gather_nchunk=64, cmax=1, mean_list=21320)),
              ops=("restrict", "assemble")),
    ], _finest(65600, ops=())),
    # -- the other side of NE <= 65536: N = 65 536 elements, m = 2: LDS accumulation.
    Case("acc_ne_max", 65536, [
        Level("m2", lambda N: (ranges_U(N, [(0, N)]), aggregates(2 * N, [2 * N])),
              _gen(T_long=True, T_chunks=32, max_row=1, max_col=131072, **_asm(True, "accumulate", acc_split=1, cmax=1, mean_list=0)),
              ops=("assemble",)),
    ], _finest(65536, ops=())),
]
CASE = {c.name: c for c in CASES}


def op_params(op):
    """(case name, level index) of every level that lists `op`."""
    return [(c.name, l) for c in CASES for l, lv in enumerate(c.all_levels()) if op in lv.ops]


@functools.lru_cache(maxsize=None)
def built_levels(name):
    c = CASE[name]
    return [lv.build(c.N) for lv in c.levels] + [(fine_U(c.N), sp.identity(2 * c.N, format="csr"))]


@functools.lru_cache(maxsize=None)
def problem(name):
    return fem1d_problem(CASE[name].N, built_levels(name)[:-1])


def solve_problem():
    """The hierarchy of the complete-solve test: N = 2048 elements; the coarse levels are nested in spirit (hats on 3 and 255
    interior vertices, slack aggregates of 2048 and 64 nodes).  Level 0 restricts through the chunked kernel (columns of
    2048 >= 1024 entries), level 1 through the row-parallel one (no column longer than 64), level 2 is the finest."""
    N = 2048
    return fem1d_problem(N, [(hats(N, 3), aggregates(2 * N, [2048, 2048])), (hats(N, 255), aggregates(2 * N, [64] * 64))])


SOLVE_PLANS = [dict(R_unit=False, T_long=True, T_chunks=1, max_col=2048), dict(R_unit=False, T_long=False, T_chunks=0, max_col=64),
               dict(R_unit=True, T_long=False, T_chunks=0, max_col=2)]


def level_R(name, level):
    R = sp.csr_matrix(problem(name).M[0].R_fine[level])
    R.sum_duplicates(); R.sort_indices()
    return R


def inputs(name, level):
    """(s, c, z0): s at scale 1e-3 -- smooth on the u columns (the derivative of u stays inside the cone on every mesh), mixed
    signs on the slack columns."""
    prob = problem(name)
    R = level_R(name, level)
    cu = built_levels(name)[level][0].shape[1]
    m = R.shape[1]
    t = (np.arange(cu) + 1.0) / (cu + 1.0)              # smooth in the column's position and zero at the Dirichlet ends
    j = np.arange(m - cu)
    s = 1e-3 * np.concatenate([np.sin(math.pi * t) * (1.0 + 0.5 * np.cos(5.0 * t)), np.cos(0.7 * j) + 0.3 * np.sin(0.01 * j * j + 1.0)])
    z0 = np.ascontiguousarray(prob.g.T).reshape(-1)
    return s, 0.1 * prob.f, z0


# ---------------------------------------------------------------------------------------------------------------------
# the gate arithmetic of csrc/problem.cpp (upload_csr), csrc/assembly_plan.cpp, csrc/panel_layout.hpp and csrc/kernels.hip, restated
# from R alone (p = 2 nodes per element, nu = 2 states)
# ---------------------------------------------------------------------------------------------------------------------

def element_columns(R, N):
    """E_a (N x m, 0/1): column j is in the column set of (element, state a)."""
    n = 2 * N
    A = sp.csr_matrix((np.ones(R.nnz), R.indices, R.indptr), shape=R.shape)
    out = []
    for a in range(2):
        B = A[a * n:(a + 1) * n]
        E = (B[0::2] + B[1::2]).tocsr()
        E.data[:] = 1.0
        out.append(E)
    return out


def restated_plan(R, N, no_mfma=False):
    p, nu = 2, 2
    m = R.shape[1]
    rowlen = np.diff(R.indptr)
    collen = np.bincount(R.indices, minlength=m) if R.nnz else np.zeros(m, dtype=int)
    max_row, max_col = int(rowlen.max()), int(collen.max())
    unit = max_row <= 1 and bool(np.all(R.data == 1.0))
    plan = dict(R_unit=unit, R_long=max_row > 64, T_long=max_col > 64, max_row=max_row, max_col=max_col,
                T_chunks=-(-max_col // CHUNK) if (max_col >= 1024 and m <= 16384) else 0, selection=unit)
    if unit:
        plan.update(acc=False, projection="none", long_lists=False, gather_nchunk=0)      # lists of one or two element blocks
        return plan
    Eu, Es = element_columns(R, N)
    cu_e, cs_e = np.asarray(Eu.sum(axis=1)).ravel().astype(int), np.asarray(Es.sum(axis=1)).ravel().astype(int)
    ct = cu_e + cs_e
    cmax, ctmax = max(1, int(max(cu_e.max(), cs_e.max()))), max(1, int(ct.max()))
    slab_est = int((ct.astype(np.int64) ** 2).sum())
    mt = m * (m + 1) // 2
    stage = p * ctmax + (nu * (nu + 1) // 2) * p * p + nu * p * ctmax + ctmax
    room = 144 * 1024 // 8 - stage
    nsplit = max(1, -(-mt // room)) if room > 0 else 1 << 20
    fits = p * ctmax <= 4 * 256 and (nu * (nu + 1) // 2) * p * p <= 3 * 256 and ctmax <= 256
    acc = m > 0 and m <= 384 and room > 0 and nsplit <= 4 and N <= 65536 and slab_est >= 16 * mt and fits
    plan.update(acc=acc, acc_split=nsplit, cmax=cmax)
    if acc:
        plan.update(projection="accumulate", long_lists=False, gather_chunk=0, gather_nchunk=0, mean_list=0)
        return plan
    E = (Eu + Es).tocsr()
    lists = (E.T @ E).tocoo()                           # entry (i, j): the elements that hold both columns = its list length
    nnz, maxlen = lists.nnz, int(lists.data.max())
    mean = slab_est // nnz
    plan.update(long_lists=mean > 48, mean_list=mean, gather_chunk=0, gather_nchunk=0)
    if mean > 48 and mean > 2048:
        chunk = max(1024, -(-maxlen // 64))
        plan.update(gather_chunk=chunk, gather_nchunk=-(-maxlen // chunk))
    ctpad = nu * (-(-cmax // 16) * 16)
    ppad = -(-p // 4) * 4
    mfma_lds = 8 * ((ppad + 1) * ctpad + (nu * p + 1) * (nu * ppad) + (ctpad + 1) // 2 + 8)
    staged_lds = 4 * 8 * (p * ctmax + (nu * (nu + 1) // 2) * p * p + nu * p * ctmax + ctmax)
    if not no_mfma and mfma_lds <= 64 * 1024 and ctpad >= 48:
        plan["projection"] = "mfma"
    else:
        plan["projection"] = "staged" if staged_lds <= 40 * 1024 else "loop"
    return plan


def list_lengths(R, N):
    """CSR (m x m) of contribution-list lengths of a general level without acc (elements that hold both columns)."""
    Eu, Es = element_columns(R, N)
    E = (Eu + Es).tocsr()
    return (E.T @ E).tocsr()


# ---------------------------------------------------------------------------------------------------------------------
# exact sums
# ---------------------------------------------------------------------------------------------------------------------

def exact_sum(*factors):
    """sum_t prod_k factors[k][t] as a Fraction: every product is formed exactly from the integer mantissas and carried on the
    common denominator 2^-emin (what sum(Fraction(a) * Fraction(b) ...) gives, without a gcd per term)."""
    if len(factors[0]) == 0:
        return Fraction(0)
    M, E = [], 0
    for f in factors:
        mant, e = np.frexp(np.asarray(f, dtype=np.float64))
        M.append((mant * 9007199254740992.0).astype(np.int64).tolist())         # |mant| < 1 with 53 bits: exact
        E = E + e.astype(np.int64) - 53
    emin = int(E.min())
    sh = (E - emin).tolist()
    tot = 0
    if len(M) == 2:
        for a, b, k in zip(M[0], M[1], sh):
            tot += (a * b) << k
    else:
        for a, b, c, k in zip(M[0], M[1], M[2], sh):
            tot += (a * b * c) << k
    return Fraction(tot) * Fraction(2) ** emin


@dataclass
class Reference:
    """Checked entries of one operation on one level.  index: flat positions in the device output; value: the exact sum
    rounded once; abssum: sum of |terms|; length: `len` of the bound; minterm: the smallest non-zero |term|; terms[k]: the
    factor arrays of entry k (kept for the mutation checks)."""
    index: np.ndarray
    value: np.ndarray
    exact: list
    abssum: np.ndarray
    length: np.ndarray
    minterm: np.ndarray
    bound: np.ndarray
    terms: list = field(repr=False, default_factory=list)

    @property
    def sensitive(self):
        return self.minterm >= SENSITIVITY * self.bound

    def ratios(self, device_values):
        """|device - reference| / bound on the entries that meet the sensitivity condition (entries with no term: exact 0)."""
        d = np.asarray(device_values)[self.index]
        err = np.abs(d - self.value)
        ok = self.sensitive
        empty = self.abssum == 0
        assert np.all(d[empty] == 0.0), "an entry with no term must be exactly zero"
        use = ok & ~empty
        return err[use] / self.bound[use]


def _reference(index, terms, lengths, rel_extra):
    value, exact, abssum, minterm = [], [], [], []
    for fs in terms:
        ex = exact_sum(*fs)
        exact.append(ex)
        value.append(float(ex))
        prod = np.abs(np.prod(np.stack(fs), axis=0)) if len(fs[0]) else np.zeros(0)
        abssum.append(float(exact_sum(*[np.abs(f) for f in fs])))
        nz = prod[prod > 0]
        minterm.append(float(nz.min()) if nz.size else math.inf)
    lengths = np.asarray(lengths, dtype=np.float64)
    abssum = np.array(abssum)
    bound = (lengths * U53 + rel_extra) * abssum
    return Reference(np.asarray(index), np.array(value), exact, abssum, lengths, np.array(minterm), bound, terms)


def _sample(count, always, seed):
    if count <= ALL_BELOW:
        return np.arange(count)
    rng = np.random.default_rng(seed)
    return np.unique(np.concatenate([rng.choice(count, SAMPLE, replace=False), np.asarray(always, dtype=np.int64)]))


def _extremes(lens):
    """longest, shortest non-empty and (if any) an empty row / column / list."""
    out = [int(np.argmax(lens))]
    pos = np.flatnonzero(lens > 0)
    if pos.size:
        out.append(int(pos[np.argmin(lens[pos])]))
    zero = np.flatnonzero(lens == 0)
    if zero.size:
        out.append(int(zero[0]))
    return out


@functools.lru_cache(maxsize=None)
def prolong_reference(name, level):
    """z + R s per row, z = z0."""
    R = level_R(name, level)
    s, _, z0 = inputs(name, level)
    lens = np.diff(R.indptr)
    rows = _sample(R.shape[0], _extremes(lens), 11)
    terms = []
    for i in rows:
        q = slice(R.indptr[i], R.indptr[i + 1])
        terms.append((np.concatenate([[1.0], R.data[q]]), np.concatenate([[z0[i]], s[R.indices[q]]])))
    return _reference(rows, terms, lens[rows] + 1, 0.0)


def oracle_ret(name, level):
    """The oracle's fp64 fine gradient D' y at z0 + R s (oracle.mgb_oracle.Barrier.f1 without its last product)."""
    from oracle import mgb_oracle as O
    prob = problem(name)
    Mo = O.OracleAMG(prob.M[0])
    B = O.Barrier(prob.Q)
    s, c, z0 = inputs(name, level)
    R = Mo.R_fine[level]
    Dz = O.apply_D(Mo.D_fine, z0 + R @ s)
    y = B._scale(Mo.w.size, O.node_eval(prob.Q, Dz, 1)) + Mo.w[:, None] * c
    ret = Mo.D_fine[0].T @ y[:, 0]
    for k in range(1, len(Mo.D_fine)):
        ret = ret + Mo.D_fine[k].T @ y[:, k]
    return np.asarray(ret).reshape(-1)


@functools.lru_cache(maxsize=None)
def restrict_reference(name, level):
    R = level_R(name, level)
    ret = oracle_ret(name, level)
    Rc = sp.csc_matrix(R)
    lens = np.diff(Rc.indptr)
    cols = _sample(R.shape[1], _extremes(lens), 12)
    terms = [(Rc.data[Rc.indptr[j]:Rc.indptr[j + 1]], ret[Rc.indices[Rc.indptr[j]:Rc.indptr[j + 1]]]) for j in cols]
    return _reference(cols, terms, lens[cols] + 2, KERNEL_RTOL)


def oracle_f1(name, level):
    from oracle import mgb_oracle as O
    prob = problem(name)
    Mo = O.OracleAMG(prob.M[0])
    s, c, z0 = inputs(name, level)
    return O.Barrier(prob.Q).f1(s, Mo.w, c, Mo.R_fine[level], Mo.D_fine, z0)


def oracle_f0(name, level):
    from oracle import mgb_oracle as O
    prob = problem(name)
    Mo = O.OracleAMG(prob.M[0])
    s, c, z0 = inputs(name, level)
    return O.Barrier(prob.Q).f0(s, Mo.w, c, Mo.R_fine[level], Mo.D_fine, z0)


def oracle_H_blk(name, level):
    """The oracle's f2 with R = I at the point z0 + R s: the broken-basis Hessian, fp64."""
    from oracle import mgb_oracle as O
    prob = problem(name)
    Mo = O.OracleAMG(prob.M[0])
    s, c, z0 = inputs(name, level)
    n2 = Mo.R_fine[level].shape[0]
    H = O.Barrier(prob.Q).f2(Mo.R_fine[level] @ s, Mo.w, c, sp.identity(n2, format="csr"), Mo.D_fine, z0)
    H = sp.coo_matrix(H)
    keep = H.data != 0.0
    return H.row[keep], H.col[keep], H.data[keep]


def oracle_f2(name, level):
    from oracle import mgb_oracle as O
    prob = problem(name)
    Mo = O.OracleAMG(prob.M[0])
    s, c, z0 = inputs(name, level)
    return sp.csr_matrix(O.Barrier(prob.Q).f2(s, Mo.w, c, Mo.R_fine[level], Mo.D_fine, z0))


@functools.lru_cache(maxsize=None)
def assemble_reference(name, level):
    """R' H_blk R on the upper triangle (i <= j) of the structural pattern: index = i * m + j.  `len` of the bound is the
    entry's contribution-list length: the elements that hold both columns (one for the single-contribution entries of a
    selection level)."""
    R = level_R(name, level)
    N = CASE[name].N
    m = R.shape[1]
    ha, hb, hv = oracle_H_blk(name, level)
    rowlen = np.diff(R.indptr)
    # every term R_ai H_ab R_bj: expand the nonzeros of H_blk over the entries of rows a and b of R
    na, nb = rowlen[ha], rowlen[hb]
    cnt = na * nb
    t_h = np.repeat(np.arange(ha.size), cnt)
    off = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    qa = R.indptr[ha[t_h]] + off // nb[t_h]
    qb = R.indptr[hb[t_h]] + off % nb[t_h]
    i, j = R.indices[qa], R.indices[qb]
    up = i <= j
    key = i[up].astype(np.int64) * m + j[up]
    fa, fh, fb = R.data[qa[up]], hv[t_h[up]], R.data[qb[up]]
    order = np.argsort(key, kind="stable")
    key, fa, fh, fb = key[order], fa[order], fh[order], fb[order]
    uniq, start = np.unique(key, return_index=True)
    end = np.append(start[1:], key.size)
    lens = list_lengths(R, N)
    if m > ALL_BELOW:
        sel = _sample(uniq.size, _extremes(end - start), 13)
        uniq, start, end = uniq[sel], start[sel], end[sel]
    terms = [(fa[a:b], fh[a:b], fb[a:b]) for a, b in zip(start, end)]
    length = np.asarray(lens[uniq // m, uniq % m]).ravel()
    return _reference(uniq, terms, length + 2, KERNEL_RTOL)


def dense_H(H, m):
    """The device's CSR Hessian as a flat dense array (index i * m + j)."""
    return np.asarray(sp.csr_matrix(H).todense()).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# vector reductions: lengths around the 256-thread block, the block cap and the grid-stride wrap
# ---------------------------------------------------------------------------------------------------------------------

def reduce_block_cap():
    """`reduce_blocks` of csrc/kernels.hip: ceil(n / 256) blocks, capped."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "multigridbarrier.jl_amd", "csrc",
                            "kernels.hip")).read()
    body = src[src.index("static int reduce_blocks(int64_t n)"):]
    mt = re.search(r"if \(b > (\d+)\) b = (\d+);", body)
    assert mt and mt.group(1) == mt.group(2)
    return int(mt.group(1))


def reduction_lengths():
    B = reduce_block_cap()
    return [1, 255, 256, 257, 256 * B - 1, 256 * B, 256 * B + 1, 2 * 256 * B + 77]      # the last: past the grid-stride wrap


def reduction_vectors(n, seed=0):
    """Mixed signs, 10^12 dynamic range, <= 26 significant bits per entry: every product a_i b_i is exact in fp64."""
    rng = np.random.default_rng(seed + n)

    def vec():
        v = rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-6.0, 6.0, n)
        mant, e = np.frexp(v)
        return np.ldexp(np.round(mant * 2.0 ** 26) / 2.0 ** 26, e)
    return vec(), vec()


# ---------------------------------------------------------------------------------------------------------------------
# worker process (environment switches are read once per process): python gate_cases.py assemble CASE LEVEL OUT.npz
#                                                                   python gate_cases.py solve OUT.npz
# ---------------------------------------------------------------------------------------------------------------------

def _worker(argv):
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if argv[0] == "assemble":
        from mgb_amd.device import DeviceProblem, HipContext
        name, level, out = argv[1], int(argv[2]), argv[3]
        prob = problem(name)
        ctx = HipContext(0)
        P = DeviceProblem(ctx, prob.M[0], prob.Q)
        H = P.f2(level, *inputs(name, level))
        np.savez(out, H=dense_H(H, H.shape[0]), plan=json.dumps(P.level_plan(level)))
        P.close()
        ctx.close()
    elif argv[0] == "solve":
        import mgb_amd as m
        from mgb_amd.device import DeviceProblem, HipContext
        prob = solve_problem()
        ctx = HipContext(0)
        P = DeviceProblem(ctx, prob.M[0], prob.Q)
        plans = [P.level_plan(l) for l in range(len(P.level_sizes))]
        P.close()
        ctx.close()
        sol = m.mgb_solve(prob)
        np.savez(argv[1], z=sol.z, its=np.asarray(sol.SOL_main["its"]), plans=json.dumps(plans))
    else:
        raise SystemExit("unknown mode")


if __name__ == "__main__":
    import sys
    _worker(sys.argv[1:])
