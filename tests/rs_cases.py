"""Shapes that make the row-stream and Gram-build kernels run their steady-state loop (helper of
tests/test_row_stream_exact_gpu.py, checked on the CPU by tests/test_rs_cases_cpu.py).  Not a test.

A workgroup of row_stream_kernel (csrc/bh_matvec.hip.h) marches over the row groups g, g + G, g + 2G, ... of R rows each
(G = gridDim.x): pass 1, 3, 5, ... computes from register buffer A and LDS slot red[0], pass 2, 4, ... from buffer B and red[1],
and every pass but the last prefetches the next group across the barrier.  Whether any of that runs is decided by the launch
geometry of csrc/bh_api.hip, which this module MIRRORS (test_rs_cases_cpu.py parses the source and fails when the mirror is
stale):

    RS_CONFIGS / pick_config    kRsConfigs / pick_config: (T, CPT, R, blocks_per_cu) by nchunks = ld / 2, ld = n rounded up to 16
    K_MAX_CHUNKS                kMaxChunks: above it (n > 16384) J is swept in column panels,
    K_PANEL_CHUNKS, K_PANEL_CFG kPanelChunks chunks (4096 columns) per launch, all with geometry kPanelCfg
    grid_for                    grid_for: min(n_cu * blocks_per_cu, number of row groups)
    GNG_BS, gram_geometry       csrc/bh_gngram.hip.h / gram_geometry: 64 x 64 blocks of G and the row slabs of a build

cases(n_cu) is written for the option blocks_per_cu = 1 (grid = n_cu whenever there are that many row groups), the smallest grid
the library offers: the row counts below are derived from R and that grid, never one worst-case height.

Coverage table — per path (geometries 0..6 and the column-panel path), with G = n_cu and N = d + q rows:

    tag   row groups           passes of workgroup 0   last group            q
    3A    2G + max(2, G/4) *   3, ends on buffer A     full                  3: d mod R != 0, the mu boundary lies inside a
                                                                                group of the third pass (R = 1: d mod R = 0 always)
    3a    2G + 1               3, ends on buffer A     1 row                 0
    2B    G + G/2              2, ends on buffer B     full                  1
    2b    2G                   2, ends on buffer B     R - 1 rows            0
    G     G                    1 (exactly the grid)    full                  0
    g     G                    1                       R - R/2 rows          2
    G1    G + 1                2 for workgroup 0 only  full                  0
    g1    G + 1                2 for workgroup 0 only  1 row                 3: the mu rows straddle the two passes
    (* the panel path takes 2G + 2: with R = 4 and n > 16384 three passes already cost 2049 x 16400 = 34 M elements — the one
       place where the ~10 M elements per case cannot be kept; every other case stays below it at 256 CUs.)

    R = 1 (geometry 6) has no partial row group: its lower-case rows are dropped.
    Each path alternates two n: the upper edge of its range and an odd n strictly inside whose ld is not a multiple of 2 T
    (lanes of the last k inactive).  The panel path has no upper edge; it takes n = 16400 (ld = 16400: four full panels and
    one of 8 chunks) and n = 17001 (ld = 17008: four full panels and one of 312 chunks).  With kPanelChunks = 2048 every n
    above 16384 needs at least five launches per sweep, so "two panels" does not exist; the read-modify-write of t_out runs
    four times per row in both.
"""
from collections import namedtuple

# (T, CPT, R, blocks_per_cu) — kRsConfigs
RS_CONFIGS = [
    (64, 1, 8, 8),
    (256, 1, 8, 4),
    (256, 2, 8, 2),
    (256, 4, 4, 2),
    (256, 8, 4, 1),
    (512, 8, 2, 1),
    (512, 16, 1, 1),
]
PICK_THRESHOLDS = [64, 256, 512, 1024, 2048, 4096]     # pick_config: nchunks <= PICK_THRESHOLDS[i] -> i, else the last geometry
K_MAX_CHUNKS = 8192
K_MAX_BLOCKS_PER_CU = 8
K_PANEL_CHUNKS = 2048
K_PANEL_CFG = 4
GNG_BS = 64
PANEL = "panel"                                        # path name of the column-panel fallback
PATHS = list(range(len(RS_CONFIGS))) + [PANEL]

# upper edge / odd inside n per path
PATH_N = {0: (128, 77), 1: (512, 301), 2: (1024, 777), 3: (2048, 1501), 4: (4096, 3001), 5: (8192, 6001), 6: (16384, 12001),
          PANEL: (16400, 17001)}

Case = namedtuple("Case", "d n q path tag")


def ld_of(n):
    return (max(n, 1) + 15) // 16 * 16


def nchunks_of(n):
    return ld_of(n) // 2


def pick_config(nchunks):
    for i, t in enumerate(PICK_THRESHOLDS):
        if nchunks <= t:
            return i
    return len(PICK_THRESHOLDS)


def path_of(n):
    """Geometry index of the single-launch sweeps of an n-column image, or PANEL."""
    nc = nchunks_of(n)
    return PANEL if nc > K_MAX_CHUNKS else pick_config(nc)


def config_of(path):
    return RS_CONFIGS[K_PANEL_CFG if path == PANEL else path]


def n_range(path):
    """(lo, hi]: the n served by a path (hi = None: unbounded)."""
    if path == PANEL:
        return 2 * K_MAX_CHUNKS, None
    edges = [0] + [2 * t for t in PICK_THRESHOLDS] + [2 * K_MAX_CHUNKS]
    return edges[path], edges[path + 1]


def panel_widths(n):
    """Chunks per launch of a column-panel sweep."""
    nc = nchunks_of(n)
    return [min(K_PANEL_CHUNKS, nc - c0) for c0 in range(0, nc, K_PANEL_CHUNKS)]


def grid_for(path, nrows, n_cu, blocks_per_cu=1):
    T, CPT, R, bpc_default = config_of(path)
    ngroups = (nrows + R - 1) // R
    bpc = blocks_per_cu if blocks_per_cu > 0 else bpc_default
    return min(n_cu * min(bpc, K_MAX_BLOCKS_PER_CU), max(ngroups, 1))


def stream_shape(path, nrows, n_cu, blocks_per_cu=1):
    """What a sweep over `nrows` rows does: dict with R, grid, ngroups, passes (of workgroup 0, the busiest), busiest (how many
    workgroups make as many passes), tail (rows of the last group) and last_pass (the pass the last group belongs to)."""
    R = config_of(path)[2]
    grid = grid_for(path, nrows, n_cu, blocks_per_cu)
    ngroups = (nrows + R - 1) // R
    passes = (ngroups + grid - 1) // grid
    return dict(R=R, grid=grid, ngroups=ngroups, passes=passes, busiest=ngroups - (passes - 1) * grid,
                tail=nrows - (ngroups - 1) * R, last_pass=(ngroups - 1) // grid + 1)


def mu_boundary(path, d, q, n_cu, blocks_per_cu=1):
    """(pass, offset inside its row group) of row d, the first row weighted by mu, in a sweep over d + q rows."""
    s = stream_shape(path, d + q, n_cu, blocks_per_cu)
    return (d // s["R"]) // s["grid"] + 1, d % s["R"]


def gram_geometry(nrows, ld, n_cu):
    """(slabs, rows per slab) of a build of G — gram_geometry of csrc/bh_api.hip."""
    nb = (ld + GNG_BS - 1) // GNG_BS
    nlb = nb * (nb + 1) // 2
    s = 1
    if nlb < n_cu:
        s = max(1, min((2 * n_cu + nlb - 1) // nlb, (nrows + 255) // 256))
    rows = (max((nrows + s - 1) // s, 1) + 15) // 16 * 16
    s = max(1, (nrows + rows - 1) // rows)
    return s, rows


def cases(n_cu):
    """The (d, n, q, path, tag) list of part B1, for a device with n_cu compute units and blocks_per_cu = 1."""
    G = n_cu
    out = []
    for path in PATHS:
        R = config_of(path)[2]
        edge, inside = PATH_N[path]
        many = 2 * G + (2 if path == PANEL else max(2, G // 4))
        rows = [("3A", many * R, 3, edge),
                ("3a", 2 * G * R + 1, 0, inside),
                ("2B", (G + G // 2) * R, 1, inside),
                ("2b", 2 * G * R - 1, 0, edge),
                ("G", G * R, 0, edge),
                ("g", G * R - R // 2, 2, inside),
                ("G1", (G + 1) * R, 0, inside),
                ("g1", G * R + 1, 3, edge)]
        for tag, nrows, q, n in rows:
            if R == 1 and tag.islower():
                continue                                # one row per group: no partial group
            out.append(Case(nrows - q, n, q, path, tag))
    return out


def describe(case, n_cu, blocks_per_cu=1):
    """One line of the per-session table: shape, geometry, passes, tail rows."""
    s = stream_shape(case.path, case.d + case.q, n_cu, blocks_per_cu)
    T, CPT, R, _ = config_of(case.path)
    bp, bo = mu_boundary(case.path, case.d, case.q, n_cu, blocks_per_cu)
    geo = "<%d,%d,%d>" % (T, CPT, R) + (" x %d panels" % len(panel_widths(case.n)) if case.path == PANEL else "")
    return ("%-2s d=%-6d n=%-5d q=%d  path %-5s %-24s grid %4d  groups %5d  passes %d (%4d workgroups)  tail %d rows%s"
            % (case.tag, case.d, case.n, case.q, case.path, geo, s["grid"], s["ngroups"], s["passes"], s["busiest"], s["tail"],
               "  mu rows from pass %d, row %d of its group" % (bp, bo) if case.q else ""))


# ------------------------------------------------------------------------------------------------------------------------------
# Shapes for the bit-exact check of G itself (part B2): chosen from gram_geometry so that they hold for any device with at least
# 24 compute units (test_rs_cases_cpu.py evaluates the conditions for 64, 256 and 304).
# ------------------------------------------------------------------------------------------------------------------------------
GramCase = namedtuple("GramCase", "d n q why")

GRAM_CASES = [
    GramCase(200, 130, 0, "one slab"),
    GramCase(997, 100, 3, "slab count set by (nrows + 255) / 256, short last slab; d % 4 = 1 and the mu rows start in the last slab"),
    GramCase(4996, 520, 4, "slab count set by the number of compute units, short last slab"),
    GramCase(10, 40, 2, "nrows < 16"),
    GramCase(2, 70, 1, "nrows < 4"),
    GramCase(3839, 100, 0, "one row below a slab boundary"),
    GramCase(3838, 100, 2, "at a slab boundary"),
    GramCase(3841, 100, 0, "one row above a slab boundary (last slab: 1 row)"),
    GramCase(300, 127, 1, "n = 64 k - 1"),
    GramCase(300, 128, 0, "n = 64 k"),
    GramCase(300, 129, 2, "n = 64 k + 1"),
    GramCase(600, 511, 0, "n = 64 k - 1, 36 lower blocks"),
    GramCase(600, 512, 1, "n = 64 k, 36 lower blocks"),
    GramCase(600, 513, 0, "n = 64 k + 1, 45 lower blocks"),
    GramCase(50, 5, 1, "n < 16"),
    GramCase(300, 15, 0, "n < 16, ld = 16"),
]
GRAM_WIDE_CASE = GramCase(300, 5001, 2, "4096 < n <= 16384: one slab, G probed with integer vectors")


def describe_gram(c, n_cu):
    s, rows = gram_geometry(c.d + c.q, ld_of(c.n), n_cu)
    return "d=%-5d n=%-5d q=%d  %d slab(s) of %d rows, last %d  (%s)" % (c.d, c.n, c.q, s, rows, c.d + c.q - (s - 1) * rows, c.why)
