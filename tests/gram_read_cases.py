"""Exact instances and a Python mirror for the Gram form read through its lower triangle (bh_hess_set_gram_read; helper of
tests/test_gram_read_gpu.py, proved on the CPU by tests/test_gram_read_cases_cpu.py).  Not a test.

    gram_symv_kernel<T, CPT, R, QUAD, VL>     csrc/bh_gramsym.hip.h      the rule which call takes it: csrc/bh_gram_read_plan.h

Instances.  J is 24 x n: row 0 has entries +-1, rows 1..23 entries in {-2, 0, 2}; C is one row in {0, +-2}; mu = 1/2.  Then
G_ij = J_0i J_0j + (a multiple of 4) + (0 or +-2) is an ODD integer for every pair: G is dense and every G_ii != 0 by construction.
No two rows of G agree (asserted).  v_i are integers, 1 <= |v_i| <= 7, from a fixed generator (not periodic in 2, 64, 256 or 512:
asserted).  Every partial sum of G, G v and v'G v, in any order, is an integer below 2^53 (gram_cases.Ledger), so the full read, the
lower read, any grid and NumPy in int64 give one bit pattern — and a dropped or doubled diagonal, an above-diagonal element let in, a
v_i / v_j mix-up or a skipped chunk gives another (FAULTS, model).

Mirror.  Workgroup b of a grid of G takes the row groups ngroups - 1 - gram_read_group(b, p, G), p = 0, 1, ... (serpentine, the
heaviest first); row i loads its
16-byte chunks 0 .. i / 2; column i + 1 of an even row is dropped.  The geometry comes from tests/rs_cases.py, which
test_rs_cases_cpu.py holds against csrc/bh_api.hip; the serpentine rule and the served widths are parsed out of csrc/ by
tests/test_gram_read_cases_cpu.py."""
import functools
from collections import namedtuple

import numpy as np

import gram_cases as gc
import rs_cases as rs

ROWS = 24
MU = 0.5
# 1, 2, 3: less than one chunk pair; 15, 16, 17: around ld = 16; then each geometry threshold and one past it; 8192: the widest served
SERVED_WIDTHS = (1, 2, 3, 15, 16, 17, 128, 129, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192)
UNSERVED_WIDTH = 8200             # geometry 6 (8192 < n <= 16384): the product kernel does not fit the register file
MAX_SERVED_CHUNKS = rs.K_MAX_CHUNKS // 2
N_CU_DESIGN = (8, 64, 256, 304)

Instance = namedtuple("Instance", "n J C mu G v y q")


def served(n):
    return rs.nchunks_of(n) <= MAX_SERVED_CHUNKS


def lower_bytes(n):
    """Bytes of G one lower-triangle launch loads: row i < n brings its chunks 0 .. i / 2 (gram_read_lower_bytes)."""
    return 16 * sum(i // 2 + 1 for i in range(n))


def operands(n):
    rng = np.random.default_rng(7000 + n)
    J = np.empty((ROWS, n))
    J[0] = rng.choice([-1.0, 1.0], n)
    J[1:] = rng.choice([-2.0, 0.0, 2.0], (ROWS - 1, n))
    C = rng.choice([-2.0, 0.0, 2.0], (1, n))
    v = rng.integers(1, 8, n).astype(np.float64) * rng.choice([-1.0, 1.0], n)
    return J, C, v


@functools.lru_cache(maxsize=4)
def instance(n):
    """The instance of width n with its exact answers, computed in int64: y = G v and q = v'G v.  Read-only."""
    J, C, v = operands(n)
    Ci, vi = C.astype(np.int64), v.astype(np.int64)
    JtJ = J.T @ J                                                    # sums of 24 integers of magnitude <= 4: exact in float64
    G2 = 2 * JtJ.astype(np.int64) + Ci.T @ Ci                        # 2 G = 2 J'J + C'C (mu = 1/2), int64 from here on
    assert np.all(G2 % 4 == 2) or n == 0                             # G odd everywhere
    Gi = G2 // 2
    yi = Gi @ vi
    qi = int(vi @ yi)
    assert int(np.abs(Gi).sum(axis=1).max()) * 7 < 2 ** 53 and abs(qi) < 2 ** 53
    G = Gi.astype(np.float64)
    y = yi.astype(np.float64)
    for a in (J, C, G, v, y):
        a.setflags(write=False)
    return Instance(n, J, C, MU, G, v, y, float(qi))


def prove(inst, led):
    """The ledger proofs for one instance: every partial sum of G, of a row of G v (and of a slab column: G is symmetric) and of
    v'G v stays below 2^53 units."""
    Jt = np.vstack([inst.J, inst.C])
    led.note("G", ROWS * 4 + 2)                                      # |G_ij| <= 1 + 23 * 4 + mu * 4, every partial sum an integer
    assert np.array_equal(inst.G, Jt.T @ (np.r_[np.ones(ROWS), inst.mu][:, None] * Jt))
    M = gc.matrix_info(inst.G)
    y = led.matvec(M, inst.v, "G v")
    assert np.array_equal(y, inst.y)
    led.note("v'G v", 2 * int(np.abs(inst.v) @ (np.abs(inst.G) @ np.abs(inst.v))))       # q_i carries the off-diagonal part twice
    return M


# ------------------------------------------------------------------------------------------------------------------- the mirror
def group(b, p, G):
    """gram_read_group of csrc/bh_gram_read_plan.h."""
    return (p + 1) * G - 1 - b if p & 1 else p * G + b


def geometry(n, n_cu, bpc=0):
    """Geometry index, (T, CPT, R) and the grid of a lower-triangle launch: launch_gram_gv_lower sweeps the n rows of G."""
    path = rs.path_of(n)
    T, CPT, R, _ = rs.config_of(path)
    return dict(path=path, T=T, CPT=CPT, R=R, grid=rs.grid_for(path, n, n_cu, bpc), ngroups=-(-n // R))


def groups_of(b, geo):
    """The row groups of workgroup b in its order: ngroups - 1 - (serpentine index), while the index is in range."""
    out, p = [], 0
    while group(b, p, geo["grid"]) < geo["ngroups"]:
        out.append(geo["ngroups"] - 1 - group(b, p, geo["grid"]))
        p += 1
    return out


def rows_of(b, n, geo):
    """The rows workgroup b sweeps, in its order."""
    return [i for g in groups_of(b, geo) for i in range(g * geo["R"], min((g + 1) * geo["R"], n))]


def chunks_loaded(i):
    return i // 2 + 1


def workgroup_bytes(b, n, geo):
    return 16 * sum(chunks_loaded(i) for i in rows_of(b, n, geo))


def group_bytes(g, n, geo):
    return 16 * sum(chunks_loaded(i) for i in range(g * geo["R"], min((g + 1) * geo["R"], n)))


FAULTS = ("diagonal dropped", "diagonal twice", "above-diagonal element let in", "v_i / v_j mix-up", "chunk skipped")


def model(inst, n_cu, bpc=0, fault=None):
    """(y, q) as the two forms of gram_symv_kernel and their reductions compute them, workgroup by workgroup and slab by slab, with
    one fault injected.  Everything is an exact integer, so the order inside a workgroup does not show; the assignment of rows to
    workgroups, the chunk rule and the diagonal rule do."""
    n, G, v = inst.n, inst.G, inst.v
    geo = geometry(n, n_cu, bpc)
    ld = rs.ld_of(n)
    Gp = np.zeros((n, ld))
    Gp[:, :n] = G
    vp = np.zeros(ld)
    vp[:n] = v
    cols = np.arange(ld)
    y = np.zeros(ld)
    q = 0.0
    for b in range(geo["grid"]):
        rows = np.array(rows_of(b, n, geo), dtype=np.int64)
        if rows.size == 0:
            continue
        loaded = (cols[None, :] // 2) <= (rows[:, None] // 2)                     # chunks 0 .. i / 2
        if fault == "chunk skipped":
            loaded &= ~((cols[None, :] // 2) == (rows[:, None] // 2 - 1))          # the chunk in front of the diagonal's
        used = loaded & (cols[None, :] <= rows[:, None])                          # column i + 1 of an even row is dropped
        if fault == "above-diagonal element let in":
            used = loaded
        X = np.where(used, Gp[rows], 0.0)
        diag = Gp[rows, rows]
        off = X.copy()
        off[np.arange(rows.size), rows] = 0.0
        dot_off = off @ vp
        dterm = diag * vp[rows]
        if fault == "diagonal dropped":
            dterm = 0.0 * dterm
        t = dot_off + dterm
        coef = vp[rows][:, None] * np.ones((1, ld))
        if fault == "v_i / v_j mix-up":
            coef = np.ones((rows.size, 1)) * vp[None, :]
        zoff = X if fault == "diagonal twice" else off
        slab = (coef * zoff).sum(axis=0)
        np.add.at(slab, rows, t)
        y += slab
        q += float(vp[rows] @ (2.0 * dot_off + (2.0 * dterm if fault == "diagonal twice" else dterm)))
    return y[:n], q
