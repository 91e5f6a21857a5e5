"""CPU proof of tests/cg_rows_cases.py, the exact instances behind tests/test_cg_rows_exact_gpu.py.

1. Exactness: every quantity the two-kernel iteration forms from the rows (t = J p, c = C p, sum t^2 + mu sum c^2, J't + C'(mu c),
   r.v, alpha, beta, gamma, w) goes through gram_cases.Ledger, which bounds the numerator of the largest partial sum any order can
   meet, in integers, and asserts 53 bits.
2. Agreement: rows_model returns the bits of gram_cases.cg_oracle (the reference's loop, pHp = dot(p, Hp)) and of
   gram_cases.cg_model on G — the row form and the reference compute the same float64 on these instances.
3. Ties: the operands of the families T, N and C2n sit exactly on their thresholds.
4. Placements: ownership rule and geometry parsed from csrc/; every placement of every design grid is a deciding index and sits
   on the edge it names.
5. Sensitivity: each fault of rows_model (a comparison turned, a run dropped from gamma, a stale w) changes the result of a case."""
import math
import os
import re

import numpy as np
import pytest

import cg_rows_cases as cr
import gram_cases as gc
import rs_cases as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")
N_CU = 256


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Two results (w, status, iters, trace rows) are the same bits."""
    return ((a[1], a[2]) == (b[1], b[2]) and np.array_equal(bits(a[0]), bits(b[0])) and a[3].shape == b[3].shape
            and np.array_equal(bits(a[3]), bits(b[3])))


def all_cases(family, n, n_cus=(N_CU,)):
    """The cases of one instance over the grids of `n_cus`, each (index, kind, side) once."""
    out, seen = [], set()
    for n_cu in n_cus:
        for bpc in gc.cg_grids(n):
            found = cr.c2n_cases(n, n_cu, bpc) if family == "C2n" else cr.placed_cases(family, n, n_cu, bpc)
            for c in found:
                if (c.index, c.kind, c.side) not in seen:
                    seen.add((c.index, c.kind, c.side))
                    out.append(c)
    if family == "C2":
        out += [cr.short_case(family, n)] + cr.n_cases(n)
    if family == "C3":
        out += [cr.short_case(family, n)] + cr.t_cases(n)
    return out


# ------------------------------------------------------------------------------------------------------ the sources (claim 4)
def test_mirror_matches_the_cg_prologue_in_the_source():
    api, mv, body, cg = _src("bh_api.hip"), _src("bh_matvec.hip.h"), _src("bh_cgfuse_body.hip.h"), _src("bh_cg.hip.h")
    # the fused shape streams d + q rows of an implicit handle, and its grid comes from that row count
    assert "p.nrows = p.gram ? H->ld : H->d + H->q_eff;" in api
    assert re.search(r"static void pcg_fused_geometry\(PcgPlan& p, int nch, int n_loop\) \{\s*p\.cfg = pick_config\(nch\);\s*p\.grid = grid_for\(p\.cfg, p\.nrows\);", api)
    # run c / CPT of p_j belongs to workgroup run % grid; the owner reads w only from iteration 2 on
    assert mv.count("if (!act[k] || ((c / CPT) % (int)G) != (int)blockIdx.x) continue;") == 1
    assert "if (f.j > 1) wk = reinterpret_cast<const double2*>(f.w)[c];" in mv
    assert "if (2 * c < f.n) gm = opmin(gm, f2b_term(vv[k].x, wk.x, lo.x, hi.x, f.atol_f2b));" in mv
    assert "if (2 * c + 1 < f.n) gm = opmin(gm, f2b_term(vv[k].y, wk.y, lo.y, hi.y, f.atol_f2b));" in mv
    assert "if (tid == 0) f.gpart[blockIdx.x] = gm;" in mv
    # the decisions
    assert "const bool solved = fabs(rtv_next) < tol_cg;                       // :747" in mv
    assert "if (CGP == 2 && g < ngroups) load_group(A, g);" in mv
    assert "if (pHp <= a.atol_neg) {" in body and "if (fabs(pHp) > a.atol_neg) step = gamma;" in body and "outside = alpha > gamma;" in body
    assert "const bool from_g = (a.j == 1 && !a.init_in_memory);" in body
    # the separate-kernel shape: vectors in registers up to 4 CG_T chunks, cg_step_kernel above
    assert int(re.search(r"constexpr int CG_T = (\d+);", cg).group(1)) == 1024
    assert "else if (nch <= 4 * CG_T) hipLaunchKernelGGL((cg_step_reg_kernel<4, PHASE>)" in api and "else hipLaunchKernelGGL((cg_step_kernel<PHASE>)" in api
    assert [rs.ld_of(n) // 2 <= 4 * 1024 for n in cr.SIZES] == [n != 8200 for n in cr.SIZES]
    # device pointers are used in place for even n and aligned buffers; the fused shape needs g readable up to ld
    assert "const bool in_place = dev && (n % 2 == 0) && aligned16(g_minor)" in api
    assert "const bool feasible = in.rs_cfg_ok && in.iterates && in.g_padded;" in _src("bh_pcg_plan.h")
    assert 4096 in cr.SIZES and rs.ld_of(4096) == 4096


def test_sizes_cover_every_geometry_and_the_grid_is_the_row_forms():
    assert [rs.path_of(n) for n in cr.SIZES] == [0, 1, 2, 3, 4, 5, 5, 6, 4]
    geo, gram = cr.rows_geometry("C2", 100, N_CU, 0), gc.cg_geometry(100, N_CU, 0)
    assert (geo["nrows"], geo["grid"], gram["grid"]) == (101, 13, 14)
    assert cr.rows_geometry("C3", 1000, N_CU, 0)["grid"] == 125 and cr.rows_geometry("C2", 1000, N_CU, 0)["grid"] == 126
    for n in cr.SIZES:
        for f in ("C2", "C3", "C2n"):
            for bpc in gc.cg_grids(n):
                g = cr.rows_geometry(f, n, N_CU, bpc)
                assert g["grid"] == min(N_CU * g["bpc"], -(-g["nrows"] // g["R"])) and g["nrows"] == n + (f != "C3")


# -------------------------------------------------------------------------------------------------------- placements (claim 4)
@pytest.mark.parametrize("n", cr.SIZES)
def test_placements_sit_on_the_edges_they_name_and_are_deciding(n):
    reserved = set(cr.rows_reserved(n))
    for family in ("C2", "C3", "C2n"):
        inst = cr.rows_instance(family, n)
        assert reserved <= set(inst.deciding)
        for i in reserved:                                               # deciding: free, g != 0 once a case adds c q, q = +-1, u = 0
            assert not inst.fix[i]
            if family == "C3":
                assert inst.g0[i] == 1.0
            else:
                assert inst.q[i] in (-1.0, 1.0) and inst.g0[i] == 0.0
        for n_cu in gc.N_CU_DESIGN:
            for bpc in gc.cg_grids(n):
                geo = cr.rows_geometry(family, n, n_cu, bpc)
                per_run = 2 * geo["CPT"]
                pl = dict(cr.rows_placements(family, n, n_cu, bpc))
                assert {0, 1, n - 1} <= set(pl) <= reserved and all(0 <= i < n for i in pl)
                if n % 2:
                    assert "half of the last chunk" in pl[n - 1] and (n - 1) % 2 == 0
                firsts = [i for i in pl if i % per_run == 0]
                lasts = [i for i in pl if i % per_run == per_run - 1 or i == n - 1]
                assert len(firsts) >= 2 and len(lasts) >= 2
                assert any("first element of run" in e for e in pl.values()) and any("last element of run" in e for e in pl.values())
                wg = gc.owner(n - 1, geo)[0]
                runs = sorted({gc.owner(i, geo)[1] for i in pl if gc.owner(i, geo)[0] == wg})
                owned = [r for r in range(wg, geo["nruns"], geo["grid"]) if r * per_run < n]
                assert runs[0] == owned[0] and runs[-1] == owned[-1] and wg * per_run in pl, (family, n, n_cu, bpc, runs, owned)
                assert (len(owned) >= 2) == (len(runs) >= 2) and (len(owned) < 2 or owned[1] in runs)


def test_default_instances_of_the_gram_module_are_unchanged():
    """reserve = () is the instance gram_cases has always built; a reserve moves only what it must."""
    for family in ("C2", "C3"):
        a, b = gc.cg_instance(family, 100), gc.cg_instance.__wrapped__(family, 100, ())
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip((a.J, a.C, a.G, a.g0, a.q), (b.J, b.C, b.G, b.g0, b.q)))
        assert np.array_equal(a.fix, b.fix) and a.deciding == b.deciding == tuple(gc.all_cg_indices(100, gc.N_CU_DESIGN))
        assert set(a.deciding) | set(cr.rows_reserved(100)) == set(cr.rows_instance(family, 100).deciding)


# ---------------------------------------------------------------------------------------- exactness and agreement (claims 1, 2)
@pytest.mark.parametrize("n", cr.SIZES)
@pytest.mark.parametrize("family", ["C2", "C3", "C2n"])
def test_rows_model_is_exact_and_is_the_oracle_bit_for_bit(family, n):
    inst = cr.rows_instance(family, n)
    op = cr.row_operator(inst)
    G = cr.dense_G(inst)
    diag = np.diag(inst.J)
    ref = np.diag(diag * diag) + (inst.mu * np.outer(inst.C[0], inst.C[0]) if inst.C.shape[0] else 0.0)
    assert np.array_equal(bits(G), bits(ref)) and np.array_equal(G, G.T)
    M = gc.matrix_info(G)
    worst, groups = {}, {}
    for c in all_cases(family, n):
        what = (c.group, c.index, c.kind, c.side)
        led = gc.Ledger()
        got = cr.rows_model(op, c.g, inst.fix, c.w_l, c.w_u, c.kappa2, led, atol=c.atol)
        assert same(got, cr.rows_oracle(c)), what
        assert same(got, gc.cg_model(M, c.g, inst.fix, c.w_l, c.w_u, c.kappa2, gc.Ledger(), atol=c.atol)), what
        w, st, it, tr = got
        assert np.all(bits(w[inst.fix]) == 0), what
        for k, b in led.bits.items():
            worst[k] = max(worst.get(k, 0), b)
        groups.setdefault(c.group, []).append((c.kind, st, it, tr.shape[0]))
        finite = np.flatnonzero(np.isfinite(c.w_l) | np.isfinite(c.w_u))
        assert list(finite) == ([c.index] if c.index >= 0 else []), what
        # what each kind must make the loop do (claim 3, the outcome side)
        if c.kind == "short":
            assert (st, it, tr.shape[0]) == (1, 1, 1) and tr[0, 2] == tr[0, 1] / 2
        elif c.kind == "half":
            assert (st, it, tr.shape[0]) == (1, 2, 2) and tr[1, 2] == tr[1, 1] / 2
        elif c.kind == "tie" and c.group in cr.PLACED:
            assert tr[1, 2] == tr[1, 1] and tr.shape[0] == (2 if family == "C2" else 3)          # gamma == alpha counts as inside
            assert tr[-1, 3] == 0.0 or st == 1
        elif c.group == "C2n":
            lam, m = gc.LAM, float(inst.q @ inst.q)
            assert (st, it, tr.shape[0]) == (2, 2, 2) and list(tr[:, 0]) == [lam * m, -72.0 * lam * m] and tr[0, 1] == 3.0 / lam
            assert math.isnan(tr[1, 1]) and tr[1, 2] == 2.0 ** -4                                   # pHp_2 < 0: the step is gamma
            bound = (c.w_u if c.side == "upper" else c.w_l)[c.index]
            assert w[c.index] == bound and np.all((w <= c.w_u) & (w >= c.w_l))                      # met exactly, from the side named
            p2 = -6.0 * inst.g0 - 12.0 * (c.g - inst.g0)                                            # -6 u - 12 c q
            w1 = -(3.0 / lam) * c.g
            assert np.array_equal(np.where(inst.fix, 0.0, w1 + 2.0 ** -4 * p2), w)
    if family == "C2":
        m = float(inst.q @ inst.q)
        kinds = {k: (st, it, rows) for k, st, it, rows in groups["N"]}
        assert kinds == {"at2": (2, 2, 2), "below2": (0, 3, 2), "at1": (2, 1, 1)}
    if family == "C3":
        kinds = {k: (st, it, rows) for k, st, it, rows in groups["T"]}
        assert kinds == {"tie": (0, 4, 3), "above": (0, 3, 2)}
    print("%s n = %d: worst numerator widths %s" % (family, n, dict(sorted(worst.items()))))
    assert max(worst.values()) <= 40, worst


# ------------------------------------------------------------------------------------------------------------- ties (claim 3)
@pytest.mark.parametrize("n", cr.SIZES)
def test_the_operands_of_t_and_n_sit_on_their_thresholds(n):
    # T: fl(kappa2 sqrt(9 k)) == r.v after iteration 2, whatever sqrt does to a perfect square, and the neighbour differs
    inst = cr.rows_instance("C3", n)
    op = cr.row_operator(inst)
    tie, above = cr.t_cases(n)
    s = cr.t_square(n)
    k = s * s
    free_g = np.where(inst.fix, 0.0, tie.g)
    assert float(free_g @ free_g) == 9.0 * k and math.sqrt(9.0 * k) == 3.0 * s == float(np.sqrt(9.0 * k))
    w, st, it, tr = cr.rows_model(op, tie.g, inst.fix, tie.w_l, tie.w_u, tie.kappa2, gc.Ledger())
    assert tr[1, 3] == 45.0 * k / 16.0 == tie.kappa2 * (3.0 * s) and tie.kappa2 == 15.0 * s / 16.0
    assert above.kappa2 * (3.0 * s) > tr[1, 3] and above.kappa2 == np.nextafter(tie.kappa2, np.inf)
    assert tr[0, 3] > above.kappa2 * (3.0 * s)                           # iteration 1 is far from the threshold
    assert (st, it) == (0, 4) and tr[2, 3] == 0.0
    diag = np.diag(inst.J)
    assert np.array_equal(np.where(inst.fix, 0.0, diag * diag * w), np.where(inst.fix, 0.0, -tie.g))      # w is the exact minimiser
    # N: atol equals the modelled pHp bit for bit
    inst = cr.rows_instance("C2", n)
    op = cr.row_operator(inst)
    at2, below2, at1 = cr.n_cases(n)
    w0, st, it, tr = cr.rows_model(op, below2.g, inst.fix, below2.w_l, below2.w_u, below2.kappa2, gc.Ledger(), atol=below2.atol)
    assert bits(tr[1, 0]) == bits(at2.atol) and bits(tr[0, 0]) == bits(at1.atol) and tr[1, 0] == tr[0, 0] / 2
    assert below2.atol < at2.atol and below2.atol == np.nextafter(at2.atol, 0.0)
    w2, st2, it2, tr2 = cr.rows_model(op, at2.g, inst.fix, at2.w_l, at2.w_u, at2.kappa2, gc.Ledger(), atol=at2.atol)
    assert (st2, it2) == (2, 2) and math.isnan(tr2[1, 2]) and math.isnan(tr2[1, 1])
    assert np.array_equal(bits(w2), bits(np.where(inst.fix, 0.0, -at2.g / (2.0 * gc.LAM)) + 0.0))          # w_1, untouched
    w1, st1, it1, tr1 = cr.rows_model(op, at1.g, inst.fix, at1.w_l, at1.w_u, at1.kappa2, gc.Ledger(), atol=at1.atol)
    assert (st1, it1) == (2, 1) and not bits(w1).any()


# ------------------------------------------------------------------------------------------------------- sensitivity (claim 5)
@pytest.mark.parametrize("n", [100, 4099])
def test_every_fault_changes_the_result_of_a_case(n):
    """n = 100: every workgroup owns several runs; n = 4099: odd, CPT = 8, the owner of the last run owns two."""
    caught = {}
    for family in ("C2", "C3", "C2n"):
        inst = cr.rows_instance(family, n)
        op = cr.row_operator(inst)
        geo = cr.rows_geometry(family, n, N_CU, 0)
        for c in all_cases(family, n):
            good = cr.rows_model(op, c.g, inst.fix, c.w_l, c.w_u, c.kappa2, gc.Ledger(), atol=c.atol)
            for fault in ("ge", "le_tol", "lt_neg", "drop_last_run", "stale_w"):
                bad = cr.rows_model(op, c.g, inst.fix, c.w_l, c.w_u, c.kappa2, cr.Unchecked(), atol=c.atol, geo=geo, fault=fault)
                if not same(good, bad):
                    caught.setdefault(fault, set()).add((c.group, c.kind, c.edge))
    assert set(caught) == {"ge", "le_tol", "lt_neg", "drop_last_run", "stale_w"}, caught
    assert {k for g, k, e in caught["ge"]} == {"tie"} and {g for g, k, e in caught["ge"]} == {"C2", "C3"}
    assert caught["le_tol"] == {("T", "tie", "|r.v| == tol_cg after iteration 2")}
    assert {(g, k) for g, k, e in caught["lt_neg"]} == {("N", "at2"), ("N", "at1")}
    assert any("last element of the last run" in e for g, k, e in caught["drop_last_run"])
    assert {g for g, k, e in caught["drop_last_run"]} == {"C2", "C3", "C2n"}
    assert {g for g, k, e in caught["stale_w"]} == {"C2", "C3", "C2n"}
