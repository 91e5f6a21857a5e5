"""Instances and a CPU model for the tests of option cauchy_block = K (tests/test_cauchy_block_cpu.py, _gpu.py).

The one-kernel row-space Cauchy search normally takes one breakpoint per launch.  With box constraints the row update of a pass does
not depend on that pass's sums, so a launch may run K advances ahead on the vector side and leave K pairs of sums; the next launch
checks the K decisions in order (csrc/bh_cauchyblock.hip.h).  `blocked_search` restates that launch structure in float64: speculate K,
verify in order, rebuild the final step from the recorded thetas when the search ends inside a block, three rotating s_c buffers,
`fixrank` written for verified advances only.  It must give the bits of refresh_cases.carried_search, whatever K."""
import math

import numpy as np

import benlsip_ref as R
import refresh_cases as rc

KS = (2, 4, 8, 16)
INT_MAX = 0x7fffffff
# every ending offset inside a block for K <= 4, the first, last and middle offsets for 8 and 16
NPASS = (1, 2, 3, 4, 5, 8, 9, 16, 17, 18, 33, 40)


# ------------------------------------------------------------------------------------------------------------------ the rule (§1)
def expected_block(form, fused, comm, refresh, n, K):
    """Effective K by the option's description: the one-kernel box form of the row-space search (form 1, `fused`), one rank, no
    re-formation of the images, n <= 4096, K >= 2 — otherwise 0."""
    return K if (form == 1 and fused and not comm and refresh == 0 and n <= 4096 and K >= 2) else 0


def pass_target(unit_target, K):
    return 0 if unit_target == 0 else 1 + (unit_target - 1) * K


def final_launch(passes, K):
    return 1 + -(-(passes - 1) // K)


# ------------------------------------------------------------------------------------------------------------------ the model (§2)
def _decide(phi_p, phi_pp, theta, ind, nfix, nmm):
    """cauchy_decide (src/basic_tralcnlss.jl:615-636): (done, err, advance, step)."""
    delta_t = (-phi_p / phi_pp) if phi_pp > 0 else 0.0
    if not (nfix < nmm):
        return 1, 0, 0, 0.0
    if phi_p >= 0:
        return 1, 0, 0, 0.0
    if phi_p < 0 and phi_pp > 0 and delta_t < theta:
        return 1, 0, 0, delta_t
    if ind < 0:
        return 1, 1, 0, 0.0
    return 0, 0, 1, theta


def _setup(J, C, mu, x, g, xlow, xupp, delta):
    n = J.shape[1]
    Jt = J if C is None or C.shape[0] == 0 else np.vstack([J, C])
    w = np.ones(Jt.shape[0])
    w[J.shape[0]:] = mu
    atol = np.sqrt(np.finfo(float).eps)
    fix = ((x - xlow) <= atol) | ((xupp - x) <= atol)                   # active_bounds! (poly:211)
    d_u = np.minimum(xupp - x, delta)
    d_l = np.maximum(xlow - x, -delta)
    return n, Jt, w, fix, d_l, d_u


def sequential_search(J, C, mu, x, g, xlow, xupp, delta):
    """refresh_cases.carried_search(refresh = 0) with the `no breakpoint left` exit of the device (ind < 0: error flag, the step as
    it stands) instead of an assertion.  Returns (s, active set, passes, err)."""
    n, Jt, w, fix, d_l, d_u = _setup(J, C, mu, x, g, xlow, xupp, delta)
    d = np.where(fix, 0.0, -g)
    s = np.zeros(n)
    td, ts = Jt @ d, np.zeros(Jt.shape[0])
    passes = 0
    while True:
        phi_p = float(np.dot(w * ts, td) + np.dot(g, d))
        phi_pp = float(np.dot(w * td, td))
        theta, ind = R.next_breakpoint(d, s, d_l, d_u, fix)
        done, err, advance, step = _decide(phi_p, phi_pp, theta, ind, int(fix.sum()), n)
        passes += 1
        if done:
            if step != 0.0:
                s = s + step * d
            return s, fix, passes, err
        s = s + theta * d
        ts = ts + theta * td
        td = td - d[ind] * Jt[:, ind]
        d[ind] = 0.0
        fix[ind] = True


def blocked_search(J, C, mu, x, g, xlow, xupp, delta, K, log=None):
    """float64 model of cauchy_block_kernel<K>'s launch structure.  Returns (s, active set from fixrank, passes, err); `log`, a dict,
    receives the launches run, the advances thrown away and the s_c buffer the result was taken from."""
    n, Jt, w, fix0, d_l, d_u = _setup(J, C, mu, x, g, xlow, xupp, delta)
    nmm = n
    fixpass = np.where(fix0, -1, INT_MAX).astype(np.int64)               # the state from which i counts as fixed
    fixrank = np.where(fix0, 0, -1)
    sbuf = [np.zeros(n), np.full(n, np.nan), np.full(n, np.nan)]         # cauchy_init_kernel: s_c = 0 in buffer 0
    # launch 0: t_d = J~ d_0, t_s = 0, the sums of state 0
    td, ts = Jt @ np.where(fix0, 0.0, -g), np.zeros(Jt.shape[0])
    sums_in = [(float(np.dot(w * ts, td)), float(np.dot(w * td, td)))]
    rec = None
    nfix, passes, bp, err, done = int(fix0.sum()), 0, 0, 0, 0
    b = 0
    while not done:
        b += 1
        a_b, a_prev = (b - 1) * K, (b - 2) * K
        s = sbuf[(b - 1) % 3].copy()
        fixed = fixpass <= a_b
        d = np.where(fixed, 0.0, -g)
        th0, ind0 = R.next_breakpoint(d, s, d_l, d_u, fixed)
        gd0 = float(np.dot(g, d))
        fin, step = -1, 0.0
        # ---- verify: passes a_{b-1}+1 .. a_{b-1}+K-1 from the record, then pass a_b from this launch's own first arg-min
        if b > 1:
            for j in range(1, K):
                if done or j > rec["valid"]:
                    continue
                q = _decide(sums_in[j - 1][0] + rec["gd"][j], sums_in[j - 1][1], rec["theta"][j], rec["ind"][j], nfix, nmm)
                passes += 1
                if q[2]:
                    nfix += 1
                    bp += 1
                    fixrank[rec["ind"][j]] = 0                           # verified advances only
                else:
                    done, fin, step, err = 1, j, q[3], err | q[1]
        if not done:
            assert b == 1 or rec["valid"] == K
            q = _decide(sums_in[-1][0] + gd0, sums_in[-1][1], th0, ind0, nfix, nmm)
            passes += 1
            if q[2]:
                nfix += 1
                bp += 1
                fixrank[ind0] = 0
            else:
                done, fin, step, err = 1, K, q[3], err | q[1]
        if done:
            if fin < K:
                # the finishing path: state a_{b-1}, the recorded thetas, d_i zeroed from its pass on
                s = sbuf[(b - 2) % 3].copy()
                d = np.where(fixpass <= a_prev, 0.0, -g)
                for j in range(fin):
                    s = s + rec["theta"][j] * d
                    d[rec["ind"][j]] = 0.0
            sbuf[b % 3] = (s + step * d) if step != 0.0 else s.copy()
            if log is not None:
                log.update(launches=b, wasted=(rec["valid"] - fin) if (rec is not None and fin < K) else 0, buffer=b % 3)
            break
        # ---- speculate K passes from state a_b; the rows follow pass by pass
        out = dict(valid=0, theta=[math.nan] * K, ind=[-1] * K, gd=[math.nan] * K)
        sums_out = []
        for j in range(K):
            if j > 0:
                fixed = fixpass <= a_b + j
                th, ind = R.next_breakpoint(d, s, d_l, d_u, fixed)
                gd = float(np.dot(g, d))
            else:
                th, ind, gd = th0, ind0, gd0
            out["theta"][j], out["ind"][j], out["gd"][j] = th, ind, gd
            if ind < 0 or not (nfix - 1 + j < nmm):
                break
            s = s + th * d
            ts = ts + th * td
            td = td - d[ind] * Jt[:, ind]
            d[ind] = 0.0
            fixpass[ind] = a_b + j + 1                                   # a speculative mark: never in fixrank
            sums_out.append((float(np.dot(w * ts, td)), float(np.dot(w * td, td))))
            out["valid"] = j + 1
        sbuf[b % 3] = s
        rec, sums_in = out, sums_out + [(math.nan, math.nan)] * (K - len(sums_out))
    return sbuf[b % 3], fixrank >= 0, passes, err


# ------------------------------------------------------------------------------------------------------------------ instances
# Each returns (J, C, mu, x, g, xlow, xupp, delta): what carried_search / blocked_search take.
def exact(rows, n, q, npass, seed=0):
    """refresh_cases.exact_instance: npass - 1 breakpoints, then an interior minimiser."""
    J, C, mu, A, x, g, xlow, xupp, delta = rc.exact_instance(rows, n, q, npass, seed=seed)
    return J, C, mu, x, g, xlow, xupp, delta


def bad(d=300):
    """refresh_cases.bad_instance: non-dyadic, 120 breakpoints, ends inside a segment."""
    J, x, g, xlow, xupp, delta = rc.bad_instance(d)
    return J, None, 0.0, x, g, xlow, xupp, delta


def all_fixed(n=6, rows=5):
    """Every variable reaches its bound before a segment holds a minimiser (J of size 2^-6: phi'' ~ 2^-12 ||d||^2, the minimiser
    near theta = 2^12, the bounds at theta <= 2^-13 n): n advances, and pass n + 1 ends on nfix == nmm."""
    rng = np.random.default_rng(77)
    J = rng.integers(-1, 2, size=(rows, n)).astype(np.float64) * 2.0 ** -6
    g = -(2.0 ** -(np.arange(n) % 3).astype(np.float64))
    xupp = (2.0 ** -13) * (rng.permutation(n) + 1) * (-g)
    return J, None, 0.0, np.zeros(n), g, -1024.0 * np.ones(n), xupp, 64.0


def stationary(n=5, rows=4):
    """g = 0: phi' = 0 >= 0 at pass 0."""
    rng = np.random.default_rng(78)
    J = rng.integers(-1, 2, size=(rows, n)).astype(np.float64)
    return J, None, 0.0, np.zeros(n), np.zeros(n), -np.ones(n), np.ones(n), 1.0


def no_breakpoint(n=5, rows=4):
    """J = 0, infinite bounds and trust region: phi' < 0, phi'' = 0 and no variable has a breakpoint — the reference indexes
    fixvars[-1] here, the device raises its error flag at pass 0."""
    g = -(2.0 ** -(np.arange(n) % 3).astype(np.float64))
    return np.zeros((rows, n)), None, 0.0, np.zeros(n), g, -np.inf * np.ones(n), np.inf * np.ones(n), np.inf


def tie_in_block(rows=40, n=24, q=3, npass=9):
    """exact(...) with the fourth breakpoint moved onto the third: at pass 2 two variables have the same theta, the smaller index
    goes first and the other follows at theta = 0 — both inside one block for every K >= 2 (passes 2 and 3)."""
    J, C, mu, x, g, xlow, xupp, delta = exact(rows, n, q, npass)
    hit = np.flatnonzero(xupp < 1024.0)
    order = hit[np.argsort(xupp[hit] / -g[hit])]
    i2, i3 = int(order[2]), int(order[3])
    xupp = xupp.copy()
    xupp[i3] = (xupp[i2] / -g[i2]) * -g[i3]
    return J, C, mu, x, g, xlow, xupp, delta


def named_cases():
    """(name, instance) of everything beyond the exact family."""
    yield "bad_instance_d300", bad(300)
    yield "all_fixed_n6", all_fixed(6)
    yield "all_fixed_n9", all_fixed(9, 7)
    yield "stationary_at_pass_0", stationary()
    yield "tie_in_block", tie_in_block()
