"""Active-set sequences for the bit-for-bit check of the box-constrained CG loop on the compact image of the free columns (helper of
tests/test_free_image_exact_gpu.py, checked on the CPU by tests/test_free_image_cases_cpu.py).  Not a test.

The loop on the compact image Jf (option free_image, pcg_run in csrc/bh_api.hip) runs row_stream_kernel and cg_reduce_update_kernel on
compact operands: the geometry is picked from the LIVE width, the row stride is the width at BUILD time rounded up to 16 (ldf), and w
reaches the caller through the slot -> column map.  Every sequence below is a list of active sets pushed to one Hessian handle under
free_image = 2 (build at the first eligible call, always move); Book MIRRORS free_image_book_build / free_image_book_move of
csrc/bh_free_image_plan.h (moves: last live tail column first, into ascending holes) — test_free_image_cases_cpu.py drives the header
itself, built into a stand-alone program, through the same sequences and compares the map after every step.  The launch geometry is the
mirror of rs_cases.py (pick_config, config_of, ld_of), not restated here.

rows_for(name, n_cu) = PASSES * n_cu * (largest R of any geometry the sequence visits) + 3 with q = 3, mu = 2 under blocks_per_cu = 1
(grid = one workgroup per compute unit): PASSES = 2 — every state makes at least two full passes, and the mu boundary lies inside a partial
last group — except for S2, whose operands are by far the largest of the module (n = 2101): it alone made the module slower than
tests/test_free_image_gpu.py, so its row count is one full pass plus the partial group (its R = 4 state still makes two full passes).

TABLE — per state (width, ldf, chunks, geometry, R, action, columns moved):

    S1  n = 301   140 144 72 1 8 build   | 139 144 72 1 8 move 1 (slot 0) | 128 144 64 0 8 move 11 (with tail slots: threshold 64 chunks
                  crossed, width = 0 mod 16) | 127 move 1 | 113 move 14 | 112 move 1 | 17 move 95 | 16 move 1 | 15 move 1 | 2 move 13 |
                  1 move 1 — the stride stays 144 throughout, geometry 0 from width 128 on
    S2  n = 2101  1030 1040 520 3 4 build | 1023 1040 512 2 8 move 7 (threshold 512) | 700 1040 352 2 8 move 323 (> 256: workgroup 0 of
                  free_image_move_kernel walks its map loop twice) | 513 1040 264 2 8 move 187 | 512 1040 256 1 8 move 1 (threshold 256)
    S3  n = 304   150 160 80 1 8 build | 149 move 1 | 144 move 5 — n == ld: device operands are used in place (projected_cg_dev)
    S4  n = 301   two constraint handles on one Hessian handle: A (width 140) build | B = A + 5 fixed: move 5 | A: a variable was freed,
                  rebuild | B: move 5 | B, the same array written again and marked dirty: use | B' (as many fixed as B, another set): rebuild
    S5  n = 77    3 16 8 0 8 build | 20 freed: 23 32 16 0 8 rebuild | 16 32 8 0 8 move 7

    Exception to "the box run ends on the boundary after at least two products": S1 at widths 2 and 1 and S5 at width 3.  With one free
    variable CG is exact after one product, so no second one exists; with two or three, the wide run itself already meets kappa2 after
    one or two products on these well-conditioned columns, and every radius that is reached at all is reached by the first step.  The
    second launch pair (p-buffer swap, gather-free S(2)) at a tiny width is covered by S1 at widths 15 to 17 and S5 at widths 16 and 23.

Bounds.  R.build_step_bounds gives finite bounds to the FIXED variables only (the reference's quirk), so with its bounds alone no CG run
ever ends on a bound of a free variable.  The "box" setting therefore takes build_step_bounds' values on the fixed variables and the same
expression, max(xlow - x, -delta) / min(xupp - x, delta), on the free ones (x = 0 there, |xlow| = xupp = XB > delta: +-delta); the radius
is the first of BOX_FACTORS x max|w| of the wide run at which the oracle ends on the boundary after at least two products (where none does — a
handful of free variables, CG is exact after as many products — the largest at which it ends there at all).  The "wide" setting is +-WIDE on the free variables.
"""
from collections import namedtuple

import numpy as np

from rs_cases import config_of, ld_of, pick_config

MU = 2.0
Q = 3
XB = 1.0e4                 # |xlow| = xupp of every variable; the fixed ones sit on xupp
WIDE = 1.0e3
KAPPA2 = 0.01
SCALE_MAX = {"S1": 3.0, "S2": 1.5, "S3": 3.0, "S4": 3.0, "S5": 3.0}      # S2 has half the rows per column of the others
C_SCALE = 0.25            # mu C'C adds three eigenvalues of a few dozen: the residual of the CG run decreases without jumps
MARGIN = 1.25              # no iteration of a wide run has |r.v| within this factor of the tolerance it is compared with
INSTANCE_SEED = {"S1": 2011, "S2": 3029, "S3": 2000, "S4": 2002, "S5": 2000}      # picked on the CPU for that margin
PASSES = {"S1": 2, "S2": 1, "S3": 2, "S4": 2, "S5": 2}      # full passes of the widest-R geometry before the partial last group
BOX_FACTORS = (0.97, 0.9, 0.8, 0.6, 0.4, 0.25)
BAND = ("reference", "C-order sums", "1024-row chunks", "rows reversed", "3 row blocks")

State = namedtuple("State", "who fix width ldf nch geometry R action k builds moves map")

# name: (n, seed, [(who, op, target width or None, slot rule)])   op: build / fix / free / same / swap
SEQS = {
    "S1": (301, 11, [("A", "build", 140, None), ("A", "fix", 139, "slot0"), ("A", "fix", 128, "tail"), ("A", "fix", 127, None),
                     ("A", "fix", 113, None), ("A", "fix", 112, None), ("A", "fix", 17, None), ("A", "fix", 16, None),
                     ("A", "fix", 15, None), ("A", "fix", 2, None), ("A", "fix", 1, None)]),
    "S2": (2101, 12, [("A", "build", 1030, None), ("A", "fix", 1023, None), ("A", "fix", 700, None), ("A", "fix", 513, None),
                      ("A", "fix", 512, None)]),
    "S3": (304, 13, [("A", "build", 150, None), ("A", "fix", 149, None), ("A", "fix", 144, "tail")]),
    "S4": (301, 14, [("A", "build", 140, None), ("B", "fix", 135, None), ("A", "back", 140, None), ("B", "back", 135, None),
                     ("B", "same", 135, None), ("Bp", "swap", 135, None)]),
    "S5": (77, 15, [("A", "build", 3, None), ("A", "free", 23, None), ("A", "fix", 16, None)]),
}

TABLE = {
    "S1": [(140, 144, 72, 1, 8, "build", 0), (139, 144, 72, 1, 8, "move", 1), (128, 144, 64, 0, 8, "move", 11), (127, 144, 64, 0, 8, "move", 1),
           (113, 144, 64, 0, 8, "move", 14), (112, 144, 56, 0, 8, "move", 1), (17, 144, 16, 0, 8, "move", 95), (16, 144, 8, 0, 8, "move", 1),
           (15, 144, 8, 0, 8, "move", 1), (2, 144, 8, 0, 8, "move", 13), (1, 144, 8, 0, 8, "move", 1)],
    "S2": [(1030, 1040, 520, 3, 4, "build", 0), (1023, 1040, 512, 2, 8, "move", 7), (700, 1040, 352, 2, 8, "move", 323),
           (513, 1040, 264, 2, 8, "move", 187), (512, 1040, 256, 1, 8, "move", 1)],
    "S3": [(150, 160, 80, 1, 8, "build", 0), (149, 160, 80, 1, 8, "move", 1), (144, 160, 72, 1, 8, "move", 5)],
    "S4": [(140, 144, 72, 1, 8, "build", 0), (135, 144, 72, 1, 8, "move", 5), (140, 144, 72, 1, 8, "build", 0), (135, 144, 72, 1, 8, "move", 5),
           (135, 144, 72, 1, 8, "use", 0), (135, 144, 72, 1, 8, "build", 0)],
    "S5": [(3, 16, 8, 0, 8, "build", 0), (23, 32, 16, 0, 8, "build", 0), (16, 32, 8, 0, 8, "move", 7)],
}


class Book:
    """Python mirror of FreeImageBook with free_image_book_build / free_image_book_move and the decision of option 2."""

    def __init__(self):
        self.present = False
        self.builds = self.moves = 0
        self.n = self.ldf = self.nfree = 0
        self.mask = None
        self.map = None

    def build(self, fix):
        fix = np.asarray(fix, dtype=bool)
        free = np.flatnonzero(~fix)                                  # the free variables in index order
        self.n, self.nfree = fix.shape[0], free.shape[0]
        self.ldf = ld_of(self.nfree)
        self.map = np.full(self.ldf, -1, dtype=np.int32)
        self.map[:self.nfree] = free
        self.mask = fix.copy()
        self.present = True
        self.builds += 1

    def move(self, fix):
        """Returns dst_of_tail (one entry per column that leaves the image)."""
        fix = np.asarray(fix, dtype=bool)
        old = self.nfree
        holes = [s for s in range(old) if fix[self.map[s]]]          # ascending
        k = len(holes)
        new = old - k
        dst = np.full(k, -1, dtype=np.int32)
        h = 0
        for t in range(old - 1, new - 1, -1):                        # last live tail column first
            var = self.map[t]
            if fix[var]:
                continue                                             # a hole in the tail: dropped with it
            dst[t - new] = holes[h]
            self.map[holes[h]] = var
            h += 1
        self.map[new:old] = -1
        self.nfree = new
        self.mask = fix.copy()
        self.moves += k
        return dst

    def push(self, fix):
        """What one eligible call does under free_image = 2: ("build" | "move" | "use", columns moved)."""
        fix = np.asarray(fix, dtype=bool)
        assert 0 < int(fix.sum()) < fix.shape[0]
        if not self.present or np.any(self.mask & ~fix):             # no image, or a variable was freed: it never grows
            self.build(fix)
            return "build", 0
        k = int(np.sum(fix & ~self.mask))
        if k == 0:
            return "use", 0
        self.move(fix)
        return "move", k


def geometry_of(width):
    """(chunks, geometry, R) of the launches that stream a compact image of this live width."""
    nch = ld_of(width) // 2
    cfg = pick_config(nch)
    return nch, cfg, config_of(cfg)[2]


_STATES = {}


def states(name):
    """The State list of a sequence: active set, expected geometry, action, counters and the mirror's map after every call."""
    if name in _STATES:
        return _STATES[name]
    n, seed, steps = SEQS[name]
    rng = np.random.default_rng(seed)
    book = Book()
    sets = {}                                                        # S4: the active set each constraint handle holds
    fix = None
    out = []
    for who, op, width, rule in steps:
        if op == "build":
            fix = np.ones(n, dtype=bool)
            fix[rng.choice(n, width, replace=False)] = False
        elif op == "fix":
            fix = fix.copy()
            w = n - int(fix.sum())
            k = w - width
            live = book.map[:book.nfree]
            must = []
            if rule == "slot0":
                must = [0]
            elif rule == "tail":
                must = [s for s in (w - 1, w - 2, w - 5) if s >= 0][:k]
            rest = [s for s in rng.permutation(w) if s not in must][:k - len(must)]
            fix[live[must + [int(s) for s in rest]]] = True
        elif op == "free":
            fix = fix.copy()
            fixed = np.flatnonzero(fix)
            fix[rng.choice(fixed, width - (n - int(fix.sum())), replace=False)] = False
        elif op == "back":
            fix = sets[who].copy()
        elif op == "same":
            fix = sets[who]                                          # the very same array, written again by the test
        elif op == "swap":                                           # as many fixed as B: A's set and five variables that B leaves free
            base, b = sets["A"], sets["B"]
            fix = base.copy()
            cand = np.flatnonzero(~b)
            fix[rng.choice(cand, int(b.sum()) - int(base.sum()), replace=False)] = True
        sets[who] = fix
        action, k = book.push(fix)
        nch, cfg, Rr = geometry_of(book.nfree)
        out.append(State(who, fix.copy(), book.nfree, book.ldf, nch, cfg, Rr, action, k, book.builds, book.moves, book.map.copy()))
    _STATES[name] = out
    return out


def rows_for(name, n_cu):
    return PASSES[name] * n_cu * max(s.R for s in states(name)) + Q


# ------------------------------------------------------------------------------------------------------------------ instances
_INST = {}


def instance(name, n_cu):
    """J (d x n, column scales 1..SCALE_MAX), C (Q x n), g of a sequence, and its oracle Hessian.  The seed is chosen so that the oracle's
    wide run never comes within MARGIN of its own convergence threshold: which iteration ends the run is then not a matter of rounding,
    on any machine's BLAS."""
    import benlsip_ref as R
    if (name, n_cu) not in _INST:
        n, seed = SEQS[name][:2]
        rows = rows_for(name, n_cu)
        d = rows - Q
        rng = np.random.default_rng(INSTANCE_SEED[name])
        scale = rng.permutation(np.geomspace(1.0, SCALE_MAX[name], n))
        J = rng.standard_normal((d, n)) / np.sqrt(d) * scale
        C = rng.standard_normal((Q, n)) * C_SCALE
        g = J.T @ rng.standard_normal(d) + 1e-3 * rng.standard_normal(n)
        _INST[(name, n_cu)] = dict(n=n, d=d, J=J, C=C, g=g, Ho=R.AlHessian(J, C, MU), A=np.zeros((0, n)))
    return _INST[(name, n_cu)]


def oracle_constraints(I, fix):
    import benlsip_ref as R
    n = I["n"]
    return R.make_mixed_constraints(I["A"], R.chol_lower(I["A"] @ I["A"].T), fix, l=-XB * np.ones(n), u=XB * np.ones(n))


def bounds(I, fix, delta=None):
    """(w_l, w_u, cons_o): delta None = wide, else the box of radius delta (module docstring)."""
    import benlsip_ref as R
    cons_o = oracle_constraints(I, fix)
    x = np.where(fix, XB, 0.0)
    w_l, w_u = R.build_step_bounds(x, cons_o, WIDE if delta is None else delta)
    r = WIDE if delta is None else delta
    w_l[~fix] = np.maximum(-XB - x[~fix], -r)
    w_u[~fix] = np.minimum(XB - x[~fix], r)
    return w_l, w_u, cons_o


_CELLS = {}


def cell(name, n_cu, k, setting, band=True):
    """The oracle's view of state k of a sequence under a bounds setting ("wide" | "box"): bounds, w, status, iters, n_hmul, the band of
    iteration counts over the re-associations of its own H*p (band = False: left out), and (box) the radius found.  Computed once."""
    import benlsip_ref as R
    from _util import oracle_iteration_band
    key = (name, n_cu, k, setting)
    if key in _CELLS:
        c = _CELLS[key]
        if band and "band" not in c:
            c["band"] = oracle_iteration_band(instance(name, n_cu)["g"], instance(name, n_cu)["Ho"], c["w_l"], c["w_u"], c["cons_o"], KAPPA2,
                                              variants=BAND)
        return c
    I = instance(name, n_cu)
    st = states(name)[k]

    def run(delta):
        w_l, w_u, cons_o = bounds(I, st.fix, delta)
        tr = R.CGTrace()
        w, s, it = R.projected_cg(I["g"], I["Ho"], w_l, w_u, cons_o, KAPPA2, trace=tr)
        return dict(w_l=w_l, w_u=w_u, cons_o=cons_o, w=w, status=int(s), iters=int(it), n_hmul=tr.n_hmul, delta=delta, rows=tr.rows)

    if setting == "wide":
        c = run(None)
        tol_cg = KAPPA2 * float(np.linalg.norm(np.where(st.fix, 0.0, I["g"])))
        c["rtv_over_tol"] = [abs(r[3]) / tol_cg for r in c["rows"]]          # what :747 compares, per iteration
    else:
        wide = cell(name, n_cu, k, "wide", band=False)
        hits = []
        for f in BOX_FACTORS:
            t = run(f * float(np.max(np.abs(wide["w"]))))
            if t["status"] == int(R.CGStatus.bound_hit):
                hits.append(t)
                if t["n_hmul"] >= 2:
                    break
        c = next((t for t in hits if t["n_hmul"] >= 2), hits[0] if hits else None)
        assert c is not None, ("no radius ends on the boundary", name, k)
    if band:
        c["band"] = oracle_iteration_band(I["g"], I["Ho"], c["w_l"], c["w_u"], c["cons_o"], KAPPA2, variants=BAND)
    _CELLS[key] = c
    return c


# ------------------------------------------------------------------------------------------- one exact iteration (integers)
EXACT_N = 301
EXACT_WIDTHS = (140, 128, 1)          # after a build, after a move that leaves width % 16 == 0, one free column
EXACT_SEED = 21
EXACT_BIG = 2.0 ** 20                 # the wide bounds: a power of two, gamma = 2^20 / max|g_f| is one correctly rounded division


def exact_jacobian(n, d):
    """proj_cases.cg_jacobian(n) (J'J = 16 I on any subset of columns) over d >= n rows, the rest zero."""
    from proj_cases import cg_jacobian
    J = np.zeros((d, n))
    J[:n] = cg_jacobian(n)
    return J


def exact_sets():
    """The three active sets (nested) and the integer g of the exact iteration; g is non-zero everywhere."""
    rng = np.random.default_rng(EXACT_SEED)
    order = rng.permutation(EXACT_N)
    sets = []
    for w in EXACT_WIDTHS:
        fix = np.ones(EXACT_N, dtype=bool)
        fix[order[:w]] = False
        sets.append(fix)
    g = rng.integers(1, 8, EXACT_N).astype(np.float64) * np.where(rng.random(EXACT_N) < 0.5, -1.0, 1.0)
    return sets, g


def exact_magnitude_bound(n=EXACT_N):
    """The largest magnitude any intermediate of the exact iteration can reach, in any summation order: entries of J are at most 4 in
    magnitude, of p = -mask(g) at most 7: |(J p)_i| <= 4 * 7 * n, and the sum of squares over at most n non-zero rows (times nothing:
    C = 0) is at most n * (28 n)^2; r'v = sum g_i^2 <= 49 n."""
    t = 4 * 7 * n
    return max(n * t * t, 49 * n)
