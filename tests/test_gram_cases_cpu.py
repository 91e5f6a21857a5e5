"""CPU proof of tests/gram_cases.py, the exact instances behind tests/test_gram_exact_gpu.py.

1. Every instance is exact: each quantity the Gram-form kernels form (CG: G, G p, p'Hp, r.v, alpha, beta, gamma, w; Cauchy: Hd,
   s'Hd, d'Hd, g'd, theta, a, B, y) is recomputed through gram_cases.Ledger, which bounds the numerator of the largest partial
   sum any order of summation can meet, in integers, and asserts 53 bits.  The only roundings left are the final quotient
   -phi'/phi'' and the product-then-sum s_c + step d behind it.
2. The oracle returns that result: R.projected_cg with the Gram-form H*v and refresh_cases.oracle_step, to the last bit of w / s, with
   status, iterations, passes, active set and (CG) the trace rows.
3. Every instance triggers the code it claims, from the geometry in the sources (parsed here; the row-stream geometry mirror of
   rs_cases.py is checked against the source by test_rs_cases_cpu.py)."""
import os
import re

import numpy as np
import pytest

import gram_cases as gc
import refresh_cases as rc
import rs_cases as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")
N_CU = 256


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ------------------------------------------------------------------------------------------------------ the sources (claim 3)
def test_mirror_matches_the_gram_kernels_in_the_source():
    api, cauchy, cgram, cgeq, gcg = _src("bh_api.hip"), _src("bh_cauchy.hip.h"), _src("bh_cauchygram.hip.h"), _src("bh_cauchygrameq.hip.h"), _src("bh_gramcg.hip.h")
    assert int(re.search(r"constexpr int CA_T = (\d+);", cauchy).group(1)) == gc.CA_T
    m = re.search(r"constexpr int NW = CA_T / 64, E = (\d+), TILE = E \* CA_T;", cgram)
    assert int(m.group(1)) == gc.CG_E and gc.TILE == gc.CG_E * gc.CA_T
    assert "auto elem = [&](int base, int k) { return base + (k >> 1) * 2 * CA_T + 2 * tid + (k & 1); };" in cgram
    assert re.search(r"if \(n <= 8 \* CA_T\) hipLaunchKernelGGL\(cauchy_gram_kernel<true>", api) and 8 * gc.CA_T == gc.TILE
    assert "if (cauchy_theta_before(t2, i2, th, ind))" in cgram
    assert "const int cpg = (ga.mA + 15) >> 4, j0 = grp * cpg;" in cgeq
    assert "const int e = lane & 15, grp = 4 * wave + (lane >> 4);" in cgeq and "const int i = block * 16 + e;" in cgeq and gc.EQ_BLOCK == 16
    assert int(re.search(r"constexpr int kCauchyGramEqRefresh = (\d+);", api).group(1)) == gc.EQ_REFRESH
    assert "const bool form_ab = (index % kCauchyGramEqRefresh) == 0;" in api and "const int rblocks = (int)(H->ld / 16)" in api
    assert "hipLaunchKernelGGL(image_b_mfma_kernel, dim3((unsigned)((n + 127) / 128)), dim3(256), 0, s, (const double*)H->G, H->ld, n," in api
    # gram_cg_kernel: the row stream runs over the ld rows of the image of G; run c / CPT of p_j belongs to workgroup run % grid
    assert "p.nrows = p.gram ? H->ld : H->d + H->q_eff;" in api
    assert "if (!act[k] || ((c / CPT) % (int)G) != (int)blockIdx.x) continue;" in gcg
    assert "const bool solved = fabs(rtv_next) < tol_cg;" in gcg and "if (NOPF && g < ngroups) load_group(A, g);" in gcg
    assert "outside = alpha > gamma;" in _src("bh_cgfuse_body.hip.h")
    for tid in range(gc.CA_T):
        for k in range(gc.CG_E):
            for base in (0, gc.TILE):
                i = base + (k >> 1) * 2 * gc.CA_T + 2 * tid + (k & 1)
                assert gc.elem_owner(i) == (base // gc.TILE, tid, tid // 64, k)


# -------------------------------------------------------------------------------------------------------- families C2 and C3
def test_cg_sizes_cover_every_geometry():
    """The sizes cover geometries 0 .. 6; at blocks_per_cu = 1 the sizes from 2050 up make three or more passes per workgroup
    (both row buffers, and a last pass that fewer workgroups make) — the smaller ones have no more row groups than twice the
    compute units."""
    assert [rs.path_of(n) for n in gc.CG_SIZES] == [0, 1, 2, 3, 4, 5, 5, 6]
    multi = []
    for n in gc.CG_SIZES:
        for bpc in gc.cg_grids(n):
            geo = gc.cg_geometry(n, N_CU, bpc)
            assert geo["ngroups"] == geo["ld"] // geo["R"] and geo["ld"] % geo["R"] == 0       # (no partial row group: ld is a multiple of 16)
            if geo["bpc"] == 1 and geo["passes"] >= 3:
                multi.append(n)
                assert geo["busiest"] < geo["grid"] or geo["ngroups"] % geo["grid"] == 0
    assert multi == [2050, 4099, 8190, 8200]
    assert gc.cg_geometry(8200, N_CU, 0)["nruns"] == 257 and gc.cg_geometry(8200, N_CU, 0)["nchunks"] % 16 == 8      # a last run of 8 chunks
    assert gc.cg_geometry(4099, N_CU, 0)["CPT"] == 8 and 4099 % 2 == 1                                                   # a last chunk of one element


@pytest.mark.parametrize("n", gc.CG_SIZES)
def test_cg_placements_sit_on_the_edges_they_name(n):
    for n_cu in gc.N_CU_DESIGN:
        for bpc in gc.cg_grids(n):
            geo = gc.cg_geometry(n, n_cu, bpc)
            per_run = 2 * geo["CPT"]
            pl = dict(gc.cg_placements(n, n_cu, bpc))
            assert {0, 1, n - 1} <= set(pl) and all(0 <= i < n for i in pl)
            firsts = [i for i in pl if i % per_run == 0]
            lasts = [i for i in pl if i % per_run == per_run - 1 or i == n - 1]
            assert len(firsts) >= 2 and len(lasts) >= 2
            wg = gc.owner(n - 1, geo)[0]
            runs = sorted({gc.owner(i, geo)[1] for i in pl if gc.owner(i, geo)[0] == wg})
            owned = [r for r in range(wg, geo["nruns"], geo["grid"]) if r * per_run < n]
            assert runs[0] == owned[0] and runs[-1] == owned[-1] and wg * per_run in pl, (n, n_cu, bpc, runs, owned)
            assert (len(owned) >= 2) == (len(runs) >= 2) and (len(owned) < 2 or owned[1] in runs)
            assert set(pl) <= set(gc.cg_instance("C2", n).deciding)
    # on the 256 compute units of the MI355X: which sizes give a workgroup more than one run of p_j
    several = [(n, bpc) for bpc in gc.cg_grids(n) if (n - 1) // (2 * gc.cg_geometry(n, N_CU, bpc)["CPT"]) >= gc.cg_geometry(n, N_CU, bpc)["grid"]]
    assert several == {100: [(100, 0), (100, 1)], 500: [(500, 0), (500, 1)], 1000: [(1000, 0), (1000, 1)], 2047: [], 2050: [], 4099: [(4099, 0)],
                       8190: [(8190, 0)], 8200: [(8200, 0)]}[n]


@pytest.mark.parametrize("n", gc.CG_SIZES)
@pytest.mark.parametrize("family", ["C2", "C3"])
def test_cg_instances_are_exact_and_the_oracle_returns_the_rational_result(family, n):
    inst = gc.cg_instance(family, n)
    # G is J'J + mu C'C: J is diagonal (J'J = diag(J_ii^2), one product per entry), C has one row (one product per entry)
    diag = np.diag(inst.J)
    assert np.count_nonzero(inst.J) == np.count_nonzero(diag) == n and inst.C.shape[0] <= 1
    G = np.diag(diag * diag)
    if inst.C.shape[0]:
        G = G + inst.mu * np.outer(inst.C[0], inst.C[0])
    assert np.array_equal(bits(G), bits(inst.G)) and np.array_equal(inst.G, inst.G.T)
    if n <= 1000:
        assert np.array_equal(bits(inst.J.T @ inst.J + inst.mu * (inst.C.T @ inst.C)), bits(inst.G))
    M = gc.matrix_info(inst.G)
    # G p by integer arithmetic, once per instance: the float product is the integer one
    e = M["e"]
    Gi = np.rint(inst.G * 2.0 ** e).astype(np.int64)
    probe = gc.cg_case(family, n, 0, "tie", "upper").g
    ep = gc.dyadic_exp(probe)
    pi = np.rint(probe * 2.0 ** ep).astype(np.int64)
    assert int(np.abs(Gi).max()) * int(np.abs(pi).max()) * n < 2 ** 62
    assert np.array_equal(inst.G @ probe, (Gi @ pi).astype(np.float64) * 2.0 ** -(e + ep))
    worst = {}
    seen = set()
    for bpc in gc.cg_grids(n):
        for c in gc.cg_cases(family, n, N_CU, bpc) + [gc.short_case(family, n)]:
            if (c.index, c.kind, c.side) in seen:
                continue
            seen.add((c.index, c.kind, c.side))
            led = gc.Ledger()
            w, st, it, tr = gc.cg_model(M, c.g, inst.fix, c.w_l, c.w_u, c.kappa2, led)
            wo, sto, ito, tro = gc.cg_oracle(c)
            assert (st, it) == (sto, ito), (c.index, c.kind, c.side)
            assert np.array_equal(bits(w), bits(wo)) and np.array_equal(bits(tr), bits(tro)), (c.index, c.kind, c.side)
            assert np.all(bits(w[inst.fix]) == 0)
            for k, b in led.bits.items():
                worst[k] = max(worst.get(k, 0), b)
            lam = gc.LAM
            alphas = ([0.5, 0.5] if family == "C2" else [0.25, 0.125, 0.5])
            if c.kind == "short":
                assert (st, it) == (1, 1) and tr.shape[0] == 1 and tr[0, 2] == tr[0, 1] / 2 and np.array_equal(w, tr[0, 2] * -np.where(inst.fix, 0.0, c.g))
            elif c.kind == "half":
                assert (st, it) == (1, 2) and tr.shape[0] == 2 and tr[1, 2] == tr[1, 1] / 2           # outside on the second iteration
                assert list(tr[:, 1] * lam) == alphas[:2]
            else:
                assert tr[1, 2] == tr[1, 1] and tr.shape[0] == len(alphas) and list(tr[:, 1] * lam) == alphas       # the tie counts as inside
                assert tr[-1, 3] == 0.0 or st == 1                                                     # r = 0 at the end, or the bound met again at step 0
                if family == "C2":
                    assert (st, it) == (0, 3) and tr[1, 3] == 0.0
            # the deciding variable decides alone, from the side the case names
            finite = np.flatnonzero(np.isfinite(c.w_l) | np.isfinite(c.w_u))
            assert list(finite) == [c.index] and np.isfinite((c.w_u if c.side == "upper" else c.w_l)[c.index])
    assert {c.side for c in gc.cg_cases(family, n, N_CU, 0) if c.kind == "tie"} == {"upper", "lower"}
    assert {c.side for c in gc.cg_cases(family, n, N_CU, 0) if c.kind == "half"} == {"upper", "lower"}
    assert max(worst.values()) <= 40, worst            # far inside the 53 bits: nothing here is close


# ------------------------------------------------------------------------------------------------------------------- family K
def test_exact_instance_order_and_theta_step():
    """order = None is the instance the other modules have always had; an explicit order is hit in that order; the finer theta
    step is for callers that ask."""
    base = rc.exact_instance(40, 48, 3, 9)
    drawn = np.random.default_rng(1000).integers(-1, 2, size=(40, 48))                  # (the first draw: J~)
    assert np.array_equal(np.vstack([base[0], base[1]]) * 8.0, drawn)
    hit = np.flatnonzero(base[7] < 1024.0)
    order = hit[np.argsort(base[7][hit] / -base[5][hit])]
    again = rc.exact_instance(40, 48, 3, 9, order=order)
    assert all(np.array_equal(a, b) for a, b in zip(base[:2] + base[3:8], again[:2] + again[3:8]))
    rev = rc.exact_instance(40, 48, 3, 9, order=order[::-1])
    assert np.array_equal(rev[0], base[0]) and list(rev[7][order] / -rev[5][order] * 2.0 ** 13) == list(range(len(order), 0, -1))
    with pytest.raises(AssertionError):
        rc.exact_instance(40, 300, 3, 130)
    fine = rc.exact_instance(40, 300, 3, 130, theta_exp=14)
    assert np.sum(fine[7] < 1024.0) == 129 and (fine[7][fine[7] < 1024.0] / -fine[5][fine[7] < 1024.0]).max() == 129 * 2.0 ** -14


def test_k_hits_straddle_the_boundaries_of_the_kernel():
    own = gc.elem_owner
    assert [own(i)[3] >> 1 for i in (1022, 1023, 1024, 1025)] == [0, 0, 1, 1] and own(1023)[1] == gc.CA_T - 1 and own(1024)[1] == 0
    assert [own(i)[2] for i in (126, 127, 128, 129)] == [0, 0, 1, 1]
    assert own(1024)[:2] == (0, 0) and own(1024)[3] == 2 and own(2)[:2] == (0, 1) and own(2)[3] == 0     # thread 0's third, thread 1's first
    assert [own(i)[0] for i in (4094, 4095, 4096)] == [0, 0, 1]
    assert [n <= gc.TILE for n in gc.K_SIZES] == [True, True, True, False, False]
    assert -(-4097 // gc.TILE) == 2 and 4097 - gc.TILE == 1 and -(-8193 // gc.TILE) == 3 and 8193 - 2 * gc.TILE == 1
    for n in gc.K_SIZES:
        assert set(gc.k_hits(n)) == {i for i in gc.K_HITS if i < n} | {n - 1}


@pytest.mark.parametrize("n", gc.K_SIZES)
def test_k_instances_are_exact_and_the_oracle_returns_the_rational_result(n):
    M, worst = None, {}
    names, ends_between = [], []
    for c in gc.k_cases(n):
        led = gc.Ledger()
        J, C, mu, A, x, g, xlow, xupp, delta = c.inst
        if M is None:
            M, J0, C0, mu0 = gc.gram_matrix(c.inst, led), J, C, mu
        assert np.array_equal(J, J0) and np.array_equal(C, C0) and mu == mu0                # one G for every case of the size
        s, fix, passes, err = gc.gram_search_model(c.inst, led, M=M)
        so, fo, po = rc.oracle_step(J, C, mu, None, x, g, xlow, xupp, delta)
        assert err == 0 and passes == po and np.array_equal(fix, fo) and np.array_equal(bits(s), bits(so)), c.name
        names.append(c.name)
        for k, b in led.bits.items():
            worst[k] = max(worst.get(k, 0), b)
        hit = np.flatnonzero(xupp < 1024.0)
        theta = xupp[hit] / -g[hit] if c.name != "stationary" else np.array([])
        if c.name.startswith("tie_"):
            # two equal thetas, and the order shows: phi' behind the tie has opposite signs for the two orders, so the search ends
            # between the two in one order and fixes both in the other
            first, second = (int(t) for t in c.name.split("_")[1:])
            assert first < second and list(hit) == [first, second] and theta[0] == theta[1] and list(np.flatnonzero(g)) == [first, second]
            pA, pB = gc.tie_states(c.inst, first, second, theta[0])[:2]
            assert (pA >= 0) != (pB >= 0)
            if pA >= 0:                                                   # the reference fixes `first`, finds phi' >= 0 and stops
                assert passes == 2 and list(np.flatnonzero(fix)) == [first]
            else:                                                         # goes on and fixes `second` too; the other order would stop
                assert passes == 3 and list(np.flatnonzero(fix)) == [first, second]
            ends_between.append(pA >= 0)
            continue
        elif c.name == "stationary":
            assert passes == 1 and not fix.any() and not s.any()
        else:
            assert passes == len(gc.k_hits(n)) + 1 and list(np.flatnonzero(fix)) == sorted(gc.k_hits(n))
        if c.name == "ends_at_phi_p_0":
            assert not np.any(g[~fix]) and np.all(s[~fix] == 0.0)                     # d = 0: the last pass found phi' = 0
        elif c.name != "stationary":
            assert np.any(s[~fix] != 0.0)                                             # an interior minimiser: one more, inexact step
    print("n = %d: ties that end between the two breakpoints: %s" % (n, ends_between))
    assert ("tie_4095_4096" in names) == (n > gc.TILE) and ("ends_at_phi_p_0" in names) == (n in (1030, 4097))
    assert max(worst.values()) <= 40, worst


def test_k_small_endings():
    for c in gc.k_all_fixed():
        led = gc.Ledger()
        J, C, mu, A, x, g, xlow, xupp, delta = c.inst
        s, fix, passes, err = gc.gram_search_model(c.inst, led)
        so, fo, po = rc.oracle_step(J, None, mu, None, x, g, xlow, xupp, delta)
        assert fix.all() and passes == c.n + 1 == po and err == 0 and np.array_equal(bits(s), bits(so)) and np.array_equal(fix, fo)
    for n in (1030, 4097):
        s, fix, passes, err = gc.gram_search_model(gc.k_no_breakpoint(n).inst, gc.Ledger())
        assert err == 1 and passes == 1 and not fix.any() and not s.any()


# ------------------------------------------------------------------------------------------------------------------- family E
def test_e_cases_cover_the_column_slices_and_blocks():
    assert sorted({gc.cpg_of(mA) for _, mA, _ in gc.E_CASES}) == [1, 2, 3, 4]
    assert [gc.cpg_of(mA) for mA in (1, 16, 17, 33, 64)] == [1, 1, 2, 3, 4]
    # some j0 + k lie past mA: at 17 inside a group (group 8 holds column 16 and nothing at k = 1) and as whole groups, at 33 as
    # whole groups only (group 10 ends on column 32)
    inside = {}
    for mA in (17, 33):
        cpg = gc.cpg_of(mA)
        past = [(grp, k) for grp in range(16) for k in range(cpg) if grp * cpg + k >= mA]
        assert any(grp * cpg >= mA for grp, k in past)
        inside[mA] = [grp for grp, k in past if grp * cpg < mA]
    assert inside == {17: [8], 33: []}
    ns = {n for n, mA, _ in gc.E_CASES if mA == 64}
    assert {271, 272, 273, 4100} <= ns and 272 % gc.EQ_BLOCK == 0 and 273 % gc.EQ_BLOCK == 1 and 271 % gc.EQ_BLOCK == 15
    assert rs.ld_of(4100) > gc.MFMA_PANEL and gc.e_instance(4100, 64, 6)[3][:, gc.MFMA_PANEL:].any()
    assert [p for _, _, p in gc.E_CASES if p - 1 >= gc.EQ_REFRESH] == [130]


@pytest.mark.parametrize("n,mA,npass", gc.E_CASES)
def test_e_instances_are_exact_and_the_oracle_returns_the_rational_result(n, mA, npass):
    inst = gc.e_instance(n, mA, npass)
    J, C, mu, A, x, g, xlow, xupp, delta = inst
    led, log = gc.Ledger(), []
    s, fix, passes, err = gc.gram_search_model(inst, led, log=log)
    so, fo, po = rc.oracle_step(J, C, mu, A, x, g, xlow, xupp, delta)
    assert err == 0 and passes == po == npass and int(fix.sum()) == npass - 1
    assert np.array_equal(fix, fo) and np.array_equal(bits(s), bits(so))
    assert log == list(range(gc.EQ_REFRESH, npass, gc.EQ_REFRESH)) and 1 + len(log) == 1 + (npass - 1) // gc.EQ_REFRESH
    assert not A[:, fix].any()                            # the equalities live on variables that stay free: y is one vector for the whole search
    assert max(led.bits.values()) <= 40, led.bits
