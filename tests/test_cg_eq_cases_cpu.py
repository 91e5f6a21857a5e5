"""CPU proof of tests/cg_eq_cases.py, the exact instances behind tests/test_cg_eq_exact_gpu.py.

1. Exactness: every quantity the kernels of the equality loop form (t = J p, c = C p, sum t^2 + mu c^2 and dot(p, Hp) — the same
   bits —, J't + C'(mu c), the per-block partials of A_free r and their sums, Linv t, Linv'u, A'y, r.v, v.v, alpha, beta, gamma,
   w, and the augmented form's B r, (L L')^-1 B r, B'y) goes through gram_cases.Ledger, which bounds the numerator of the largest
   partial sum any order can meet, in integers, and asserts 53 bits.  The worst width is printed and bounded.
2. Agreement: eq_model returns the bits of the oracle's projected_cg (the reference's loop with its own augmented factor).
3. Ties: the operands of T, N and EC2n sit exactly on their thresholds, the one-ulp neighbours on the other side.
4. Placements: geometry and ownership rules parsed from csrc/; every placement of every design grid is a deciding index on the
   edge it names, inside a support or outside as claimed; the supports of A cover the blocks cg_eq_cases.wanted_blocks lists.
5. Sensitivity: each fault of eq_model (a comparison turned, a partial block dropped, a stale y, a run dropped from gamma)
   changes the result of a case."""
import math
import os

import numpy as np
import pytest

import benlsip_ref as R
import cg_eq_cases as ce
import gram_cases as gc
import rs_cases as rs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")
N_CU = 256
WORST_BITS = 30                          # bound on the ledger's worst numerator width (measured: 24, at mt = 256)


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Two results (w, status, iters, trace rows) are the same bits."""
    return ((a[1], a[2]) == (b[1], b[2]) and np.array_equal(bits(a[0]), bits(b[0])) and a[3].shape == b[3].shape
            and np.array_equal(bits(a[3]), bits(b[3])))


def all_cases(n, mA, n_cus=(N_CU,)):
    """The cases of one (n, mA) over the grids of `n_cus`, each (group, index, kind, side) once."""
    out, seen = [], set()
    for n_cu in n_cus:
        for bpc in gc.cg_grids(n):
            for c in ce.placed_cases(n, mA, n_cu, bpc) + ce.ec2n_cases(n, mA, n_cu, bpc):
                if (c.group, c.index, c.kind, c.side) not in seen:
                    seen.add((c.group, c.index, c.kind, c.side))
                    out.append(c)
    out += [ce.short_case(n, mA)] + ce.n_cases(n, mA)
    if (n, mA) in ce.T_TABLE:
        out += ce.t_cases(n, mA)
    return out


# ------------------------------------------------------------------------------------------------------ the sources (claim 4)
def test_mirror_matches_the_equality_kernels_in_the_source():
    api, mv, body, prj, plan = _src("bh_api.hip"), _src("bh_matvec.hip.h"), _src("bh_cgfuse_body.hip.h"), _src("bh_proj.hip.h"), _src("bh_pcg_plan.h")
    # the stream: d + q rows of the implicit handle; run c / CPT of p_j belongs to workgroup run % grid
    assert "p.nrows = p.gram ? H->ld : H->d + H->q_eff;" in api
    assert mv.count("if (!act[k] || ((c / CPT) % (int)G) != (int)blockIdx.x) continue;") == 1
    # the update kernel: 16 chunks per workgroup, one partial block of A_free r each; rows rl, rl + 16, rl + 32, rl + 48
    assert "p.nblk = (nch + 15) / 16;" in api and "const int c = blockIdx.x * 16 + cl;" in body
    assert "for (int k = 0; k < 4; ++k) arow[k] = A2[(int64_t)min(rl + 16 * k, a.mA - 1) * ldA2 + cc];" in body
    assert "const int i = rl + 16 * k;" in body and "if (i < a.mA) {" in body
    assert "if (cl == 0) a.tpart[(int64_t)blockIdx.x * a.mA + i] = prod;" in body
    assert "vk.x = (fr.x >= 0) ? 0.0 : rk.x;" in body and "if (GEN) rsm[cl] = vk;" in body
    assert "if (pHp <= a.atol_neg) {" in body and "if (fabs(pHp) > a.atol_neg) step = gamma;" in body and "outside = alpha > gamma;" in body
    assert ce.UPD_CHUNKS == 16 and ce.BLOCK == 32
    # the projection kernel: 64 chunks per workgroup; wave rg folds the blocks [rg per, min(nblk, rg per + per)) in batches of 32
    assert "const int c = blockIdx.x * 64 + cl;" in prj
    assert "const int per = (a.tpart_nblk + 3) / 4;" in prj and "const int b0 = rg * per, b1 = min(a.tpart_nblk, b0 + per);" in prj
    assert "for (int b = b0 + 32; b < b1; b += 32) {" in prj and "if (b0 + k < b1) acc += x0[k];" in prj and "if (b + k < b1) acc += x[k];" in prj
    assert "if (rg == 0) ts[cl] = (tq[0][cl] + tq[1][cl]) + (tq[2][cl] + tq[3][cl]);" in prj
    assert "const double v0 = (fr.x >= 0 || j0 >= a.n) ? 0.0 : rk.x - tx;" in prj
    assert "pa.tpart = P->tpart; pa.tpart_nblk = nblk;" in api and "pa.tpart = P->tw; pa.tpart_nblk = 1;" in api
    assert "p.nch_v = p.sel.gen_linv ? nch : (n_loop + 1) / 2;" in api and "p.nrv = p.sel.fuse_gen ? (p.nch_v + 63) / 64 : p.nblk;" in api
    assert (ce.PRJ_CHUNKS, ce.PRJ_BATCH) == (64, 32)
    # the exit test of the prologue
    assert "const bool solved = fabs(rtv_next) < tol_cg;                       // :747" in mv
    # the rule: three / four kernels up to 64 equalities in the reduced form, no refinement for one equality
    assert "const bool fuse_gen = !box && cg_fused >= 1 && in.reduced && in.mA <= 64 && in.tpart && in.lda_is_ld && (!in.gram_handle || in.W);" in plan
    assert "o.linv_refine = gen_linv && in.linv_refine != 0 && in.M_valid && in.mA >= 2;" in plan
    assert "o.cg_kernels = (box ? 2 : gen_linv ? 3 : 4) + (rccl_gen ? 1 : 0);" in plan
    # the separate shape: vectors in registers up to 4 CG_T chunks
    assert "else if (nch <= 4 * CG_T) hipLaunchKernelGGL((cg_step_reg_kernel<4, PHASE>)" in api and "else hipLaunchKernelGGL((cg_step_kernel<PHASE>)" in api
    assert [rs.ld_of(n) // 2 <= 4 * 1024 for n in ce.SIZES] == [n != 8200 for n in ce.SIZES]


def test_every_size_reaches_the_geometry_it_is_there_for():
    bg = {n: ce.block_geometry(n) for n in ce.SIZES}
    assert [(bg[n]["nblk"], bg[n]["per"], bg[n]["batches"], bg[n]["nprj"]) for n in ce.SIZES] == \
        [(4, 1, 1, 1), (64, 16, 1, 16), (65, 17, 1, 17), (128, 32, 1, 32), (129, 33, 2, 33), (257, 65, 3, 65)]
    assert [rs.path_of(n) for n in ce.SIZES] == [0, 3, 4, 4, 5, 6]
    assert [bg[n]["nch"] % 16 for n in ce.SIZES] == [8, 0, 8, 0, 8, 8]          # the last block of A_free r: half full, or full
    assert bg[2050]["quarters"][3] == (51, 65) and bg[4099]["quarters"] == [(0, 33), (33, 66), (66, 99), (99, 129)]
    assert rs.ld_of(4096) == 4096 and [n % 2 for n in ce.SIZES] == [0, 1, 0, 0, 1, 0]
    assert sorted({n for n, _ in ce.TABLE}) == list(ce.SIZES) and {mA for _, mA in ce.TABLE} == set(ce.MAS) | {3}
    assert set(ce.T_TABLE) <= set(ce.TABLE) and {ce.eq_instance(n, mA, "T").mt for n, mA in ce.T_TABLE} == {12, 48, 192}
    geo = ce.eq_geometry(100, N_CU, 0)
    assert (geo["nrows"], geo["grid"]) == (101, 13) and geo["nruns"] > geo["grid"]           # a workgroup owns several runs


# --------------------------------------------------------------------------------------------------- the instances (claim 4)
@pytest.mark.parametrize("n,mA", ce.TABLE)
def test_instance_is_the_family_the_docstring_states(n, mA):
    for kind in ("EC2",) + (("T",) if (n, mA) in ce.T_TABLE else ()):
        inst = ce.eq_instance(n, mA, kind)
        A = ce.dense_A(inst)
        free = ~inst.fix
        assert int(inst.fix.sum()) == 2 and np.all(inst.g0[inst.fix] == 1.0) and not A[:, inst.fix].any()
        assert np.array_equal(A @ A.T, 4.0 * np.eye(mA)) and np.all(np.abs(A).sum(axis=1) == 4) and np.all(np.abs(A).sum(axis=0) <= 1)
        assert np.array_equal(A @ inst.q, 2.0 * np.ones(mA))
        on = np.abs(A).sum(axis=0) > 0
        assert np.all((inst.q[on] == 0.0) | (inst.q[on] == A.sum(axis=0)[on]))                              # q = the row's sign, or 0
        assert int(np.count_nonzero(inst.q[on])) == 2 * mA and int(np.count_nonzero(inst.q[~on])) == inst.Q and not inst.q[inst.fix].any()
        assert np.array_equal(inst.qt, inst.q - A.T @ (A @ inst.q) / 4.0) and np.all(np.abs(inst.qt[on]) == 0.5)
        assert float(inst.qt @ inst.qt) == inst.mt == mA + inst.Q
        assert float(inst.u @ inst.u) == 2.0 * inst.mt and float(inst.u @ inst.qt) == 0.0 and not (A @ inst.u).any() and not inst.u[on].any()
        assert set(np.abs(inst.z)) <= {0.5, 1.0, 1.5}
        assert np.array_equal(np.where(free, inst.g0, 0.0), inst.u + A.T @ inst.z)
        if kind == "EC2":
            assert inst.mt & (inst.mt - 1) == 0 and inst.mt >= 2 * mA + 8 and 3.0 * ce.LAM / inst.mt * inst.mt == 3.0 * ce.LAM
        else:
            k = round(math.log(inst.mt / 3, 4))
            assert inst.mt == 3 * 4 ** k and ce.mu_of(inst) == ce.LAM / 4 ** k
        L = ce.factor_aug(inst)
        assert np.array_equal(L, np.diag(np.concatenate([2.0 * np.ones(mA), np.ones(2)])))


@pytest.mark.parametrize("n,mA", ce.TABLE)
def test_supports_cover_the_blocks_that_can_be_dropped(n, mA):
    inst = ce.eq_instance(n, mA)
    bg = ce.block_geometry(n)
    blocks = inst.S // ce.BLOCK
    assert all(len(set(row)) == 4 for row in blocks.tolist())                    # a row's entries sit in four different blocks
    cols = set(inst.S.ravel().tolist())
    assert {0, n - 1} <= cols
    assert (n - 1) // 2 // ce.PRJ_CHUNKS == bg["nprj"] - 1                       # column n - 1: the last projection workgroup
    assert (n - 1) // ce.BLOCK == bg["nblk"] - 1                                 # ... and the last partial block
    hit = set(blocks.ravel().tolist())
    wanted = ce.wanted_blocks(n)
    if mA == 1:
        q0, q1 = bg["quarters"][0], bg["quarters"][1]
        assert {0, q0[1] - 1, q1[0], bg["nblk"] - 1} <= hit
    else:
        assert set(wanted) <= hit, sorted(set(wanted) - hit)
        for b0, b1 in bg["quarters"]:
            assert b0 in hit and b1 - 1 in hit
        if n > 4096:
            assert max(hit) >= 128 and 32 in hit
    if n == 8200 and mA > 1:
        assert {32, 64} <= hit                                                   # the first block of the second and of the third batch


@pytest.mark.parametrize("n", ce.SIZES)
def test_placements_sit_on_the_edges_they_name_and_are_deciding(n):
    reserved = set(ce.eq_reserved(n))
    for mA in [m for nn, m in ce.TABLE if nn == n]:
        inst = ce.eq_instance(n, mA)
        cols = set(inst.S.ravel().tolist())
        assert set(inst.inside) | set(inst.outside) == reserved and not set(inst.inside) & set(inst.outside)
        assert {0, n - 1} <= set(inst.inside) and (mA == 1) == (len(inst.inside) == 2)
        for i in reserved:                                               # deciding: free, u = 0, qt = +-1 outside, +-1/2 inside
            assert not inst.fix[i] and inst.u[i] == 0.0 and (i in cols) == (i in inst.inside)
            assert abs(inst.qt[i]) == (0.5 if i in inst.inside else 1.0)
        combos = set()
        for c in ce.placed_cases(n, mA, N_CU, 0):
            combos.add((c.inside, c.kind, c.side))
        assert len(combos) == 8, (n, mA, sorted(combos))                 # tie and half, from w_u and w_l, inside a support and outside
    for n_cu in gc.N_CU_DESIGN:
        for bpc in gc.cg_grids(n):
            geo = ce.eq_geometry(n, n_cu, bpc)
            assert geo["grid"] == min(n_cu * geo["bpc"], -(-(n + 1) // geo["R"])) and geo["nrows"] == n + 1
            per_run = 2 * geo["CPT"]
            pl = dict(ce.eq_placements(n, n_cu, bpc))
            assert {0, 1, n - 1} <= set(pl) <= reserved
            if n % 2:
                assert "half of the last chunk" in pl[n - 1]
            assert len([i for i in pl if i % per_run == 0]) >= 2 and len([i for i in pl if i % per_run == per_run - 1 or i == n - 1]) >= 2
            wg = gc.owner(n - 1, geo)[0]
            runs = sorted({gc.owner(i, geo)[1] for i in pl if gc.owner(i, geo)[0] == wg})
            owned = [r for r in range(wg, geo["nruns"], geo["grid"]) if r * per_run < n]
            assert runs[0] == owned[0] and runs[-1] == owned[-1] and wg * per_run in pl, (n, n_cu, bpc, runs, owned)
            assert (len(owned) >= 2) == (len(runs) >= 2) and (len(owned) < 2 or owned[1] in runs)


# ---------------------------------------------------------------------------------------- exactness and agreement (claims 1, 2)
def test_structured_product_is_the_oracles_on_the_dense_jacobian():
    """eq_oracle multiplies with the diagonal of J; on the dense J the reference's own hmul gives the same bits, case by case."""
    for n, mA in ((100, 1), (100, 3)):
        inst = ce.eq_instance(n, mA)
        J = ce.dense_J(inst)
        for c in all_cases(n, mA):
            Ho = R.AlHessian(J, ce.instance_of(c).q.reshape(1, n), c.mu)                  # (T: its own q)
            assert same(ce.eq_oracle(c), ce.eq_oracle(c, hmul_fn=R.hmul, H=Ho)), (n, mA, c.group, c.kind, c.index)


@pytest.mark.parametrize("n,mA", ce.TABLE)
def test_eq_model_is_exact_and_is_the_oracle_bit_for_bit(n, mA):
    inst = ce.eq_instance(n, mA)
    A = ce.dense_A(inst)
    worst, groups = {}, {}
    lam, mt = ce.LAM, inst.mt
    for c in all_cases(n, mA, gc.N_CU_DESIGN):
        what = (c.group, c.index, c.kind, c.side)
        led = gc.Ledger()
        got = ce.eq_model(ce.instance_of(c), c, led)
        assert same(got, ce.eq_oracle(c)), what
        w, st, it, tr = got
        ci = ce.instance_of(c)                                                     # (T: its own supports)
        assert np.all(bits(w[ci.fix]) == 0) and not ((A if ci is inst else ce.dense_A(ci)) @ w).any(), what      # fixed components +0.0, A w == 0
        for k, b in led.bits.items():
            worst[k] = max(worst.get(k, 0), b)
        groups.setdefault(c.group, []).append((c.kind, st, it, tr.shape[0]))
        finite = np.flatnonzero(np.isfinite(c.w_l) | np.isfinite(c.w_u))
        assert list(finite) == ([c.index] if c.index >= 0 else []), what
        if c.group in ("EC2", "N") or c.group == "T":
            m = ce.instance_of(c).mt
            assert tr[0, 0] == 6.0 * lam * m and (tr.shape[0] < 2 or tr[1, 0] == 3.0 * lam * m)
        if c.kind == "short":
            assert (st, it, tr.shape[0]) == (1, 1, 1) and tr[0, 2] == tr[0, 1] / 2
        elif c.kind == "half":
            assert (st, it, tr.shape[0]) == (1, 2, 2) and tr[1, 2] == tr[1, 1] / 2 and tr[1, 3] == 1.5 * mt
        elif c.kind == "tie" and c.group == "EC2":
            assert (st, it, tr.shape[0]) == (0, 3, 2) and tr[1, 2] == tr[1, 1] == 1.0 / 32.0 and tr[1, 3] == 0.0 and tr[0, 3] == 1.5 * mt
        elif c.group == "EC2n":
            assert (st, it, tr.shape[0]) == (2, 2, 2) and list(tr[:, 0]) == [lam * mt, -72.0 * lam * mt] and tr[0, 1] == 3.0 / lam
            assert math.isnan(tr[1, 1]) and tr[1, 2] == 2.0 ** -4
            bound = (c.w_u if c.side == "upper" else c.w_l)[c.index]
            assert w[c.index] == bound and np.all((w <= c.w_u) & (w >= c.w_l))
    kinds = {k: (st, it, rows) for k, st, it, rows in groups["N"]}
    assert kinds == {"at2": (2, 2, 2), "below2": (0, 3, 2), "at1": (2, 1, 1)}
    if (n, mA) in ce.T_TABLE:
        kinds = {k: (st, it, rows) for k, st, it, rows in groups["T"]}
        assert kinds == {"tie": (0, 3, 2), "above": (0, 2, 1)}
    print("EC2 n = %d mA = %d: worst numerator widths %s" % (n, mA, dict(sorted(worst.items()))))
    for must in ("t = J p", "sum t^2", "dot(p, Hp)", "A_free r", "Linv t", "Linv'u", "A'y", "r.v", "v.v", "A r", "(L L')^-1 B r", "B'y", "gamma"):
        assert must in worst, must
    assert max(worst.values()) <= WORST_BITS, worst


# ------------------------------------------------------------------------------------------------------------- ties (claim 3)
@pytest.mark.parametrize("n,mA", ce.T_TABLE)
def test_the_operands_of_t_sit_on_the_threshold(n, mA):
    inst = ce.eq_instance(n, mA, "T")
    tie, above = ce.t_cases(n, mA)
    s = math.isqrt(3 * inst.mt)
    v1 = inst.u + inst.qt
    assert float(v1 @ v1) == 3.0 * inst.mt and math.sqrt(3.0 * inst.mt) == s == float(np.linalg.norm(v1))
    w, st, it, tr = ce.eq_model(inst, tie, gc.Ledger())
    assert tr[0, 3] == 1.5 * inst.mt == tie.kappa2 * s and tie.kappa2 == s / 2.0
    assert above.kappa2 * s > tr[0, 3] and above.kappa2 == np.nextafter(tie.kappa2, np.inf)
    assert (st, it) == (0, 3) and tr[1, 3] == 0.0
    w2, st2, it2, tr2 = ce.eq_model(inst, above, gc.Ledger())
    assert (st2, it2, tr2.shape[0]) == (0, 2, 1) and np.array_equal(bits(w2), bits(np.where(inst.fix, 0.0, -v1 / 32.0) + 0.0))


@pytest.mark.parametrize("n,mA", ce.TABLE)
def test_the_operands_of_n_sit_on_their_thresholds(n, mA):
    inst = ce.eq_instance(n, mA)
    at2, below2, at1 = ce.n_cases(n, mA)
    w0, st, it, tr = ce.eq_model(inst, below2, gc.Ledger())
    assert bits(tr[1, 0]) == bits(at2.atol) and bits(tr[0, 0]) == bits(at1.atol) and tr[1, 0] == tr[0, 0] / 2
    assert below2.atol < at2.atol and below2.atol == np.nextafter(at2.atol, 0.0)
    w2, st2, it2, tr2 = ce.eq_model(inst, at2, gc.Ledger())
    assert (st2, it2) == (2, 2) and math.isnan(tr2[1, 2]) and math.isnan(tr2[1, 1])
    v1 = inst.u + inst.qt
    assert np.array_equal(bits(w2), bits(np.where(inst.fix, 0.0, -v1 / 32.0) + 0.0))           # w_1, untouched
    w1, st1, it1, tr1 = ce.eq_model(inst, at1, gc.Ledger())
    assert (st1, it1) == (2, 1) and not bits(w1).any()


# ------------------------------------------------------------------------------------------------------- sensitivity (claim 5)
@pytest.mark.parametrize("n,mA", [(100, 3), (4099, 17), (8200, 64)])
def test_every_fault_changes_the_result_of_a_case(n, mA):
    """(100, 3): every stream workgroup owns several runs; (4099, 17): the second batch of partial blocks; (8200, 64): three."""
    inst = ce.eq_instance(n, mA)
    geo = ce.eq_geometry(n, N_CU, 0)
    cases = all_cases(n, mA)
    good = [ce.eq_model(ce.instance_of(c), c, gc.Ledger()) for c in cases]
    caught = {}
    for c, ok in zip(cases, good):
        for fault in ("ge", "le_tol", "stale_y", "drop_last_run"):
            bad = ce.eq_model(ce.instance_of(c), c, ce.cr.Unchecked(), geo=geo, fault=fault)
            if not same(ok, bad):
                caught.setdefault(fault, set()).add((c.group, c.kind, c.edge))
    assert set(caught) == ({"ge", "stale_y", "drop_last_run"} | ({"le_tol"} if (n, mA) in ce.T_TABLE else set())), caught
    assert {(g, k) for g, k, e in caught["ge"]} == {("EC2", "tie")}
    if (n, mA) in ce.T_TABLE:
        assert caught["le_tol"] == {("T", "tie", "|r.v| == tol_cg after iteration 1")}
    assert any("last element of the last run" in e for g, k, e in caught["drop_last_run"])
    assert {g for g, k, e in caught["drop_last_run"]} == {"EC2", "EC2n"}
    # a stale y shows in every call that takes a second projection
    assert {(c.group, c.kind) for c, ok in zip(cases, good) if ok[3].shape[0] >= 2 or ok[1] == 0} - {("N", "at2")} <= {(g, k) for g, k, e in caught["stale_y"]}
    # every wanted block, dropped from A_free r, changes the bits of every call that projects a second time
    twice = [(c, ok) for c, ok in zip(cases, good) if c.kind in ("tie", "below2")][:3]
    for b in ce.wanted_blocks(n):
        for c, ok in twice:
            bad = ce.eq_model(ce.instance_of(c), c, ce.cr.Unchecked(), geo=geo, fault="drop_block", fault_block=b)
            assert not same(ok, bad), (b, c.group, c.kind)
