"""tests/rs_cases.py against the source it mirrors, and against the coverage it promises.

1. The geometry list RsGeoms (kRsConfigs is built from it), pick_config, kMaxChunks, kMaxBlocksPerCu, kPanelChunks, kPanelCfg, the
   switch of with_rs_geom, grid_for and gram_geometry are parsed out of csrc/bh_api.hip, GNG_BS out of csrc/bh_gngram.hip.h: a retuned geometry
   must be carried over to the mirror, or tests/test_row_stream_exact_gpu.py would silently fall back to single-pass shapes.
2. For 256 compute units (MI355X) and two other counts the conditions of the coverage table in rs_cases.py are evaluated from
   the mirror: per path both n, passes ending on either register buffer, the grid-sized and grid + 1 row-group counts, full and
   partial last groups, the mu boundary inside a later pass; for the Gram build the slab situations of GRAM_CASES."""
import os
import re

import pytest

import rs_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _const(text, name):
    m = re.search(r"constexpr\s+\w+\s+%s\s*=\s*(\d+)\s*;" % name, text)
    assert m, "constant %s not found" % name
    return int(m.group(1))


def _body(text, signature_regex):
    """Text between the braces of the function whose head matches the regex, comments dropped, whitespace squeezed."""
    m = re.search(signature_regex, text)
    assert m, signature_regex
    i = text.index("{", m.end() - 1)
    depth, j = 0, i
    while True:
        depth += {"{": 1, "}": -1}.get(text[j], 0)
        if depth == 0:
            break
        j += 1
    body = re.sub(r"//[^\n]*", "", text[i + 1:j])
    return " ".join(body.split())


def test_mirror_matches_the_launch_geometry_in_the_source():
    api = _src("bh_api.hip")
    # the one list of geometries: kRsConfigs is built from it, every launcher reaches it through with_rs_geom
    m = re.search(r"using\s+RsGeoms\s*=\s*std::tuple<(.*?)\n\s*>;", api, flags=re.S)
    assert m, "RsGeoms not found"
    rows = [tuple(int(x) for x in r) for r in re.findall(r"RsGeom<\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*>", m.group(1))]
    assert rows == rc.RS_CONFIGS
    assert "constexpr auto kRsConfigs = rs_config_table(RsGeoms{});" in api
    assert "RsConfig{G::T, G::CPT, G::R, G::blocks_per_cu}..." in api
    # pick_config: a chain of `if (nchunks <= t) return i;` and a final return
    body = _body(api, r"int\s+pick_config\s*\(\s*int\s+nchunks\s*\)\s*\{")
    chain = [(int(t), int(i)) for t, i in re.findall(r"if \(nchunks <= (\d+)\) return (\d+);", body)]
    assert chain == list(zip(rc.PICK_THRESHOLDS, range(len(rc.PICK_THRESHOLDS))))
    rest = re.sub(r"if \(nchunks <= \d+\) return \d+;", "", body).strip()
    assert rest == "return %d;" % len(rc.PICK_THRESHOLDS), rest
    assert len(rc.RS_CONFIGS) == len(rc.PICK_THRESHOLDS) + 1
    assert _const(api, "kMaxChunks") == rc.K_MAX_CHUNKS
    assert _const(api, "kMaxBlocksPerCu") == rc.K_MAX_BLOCKS_PER_CU
    assert _const(api, "kPanelChunks") == rc.K_PANEL_CHUNKS
    assert _const(api, "kPanelCfg") == rc.K_PANEL_CFG
    assert _const(_src("bh_gngram.hip.h"), "GNG_BS") == rc.GNG_BS
    # the switch that turns an index into a geometry walks the list in order, the last entry as the default; no triple is
    # written anywhere else (a second table could drift from the first)
    body = _body(api, r"void\s+with_rs_geom\s*\(\s*int\s+cfg\s*,")
    inst = re.findall(r"(case (\d+)|default): f\(std::tuple_element_t<(\d+), RsGeoms>\{\}\); break;", body)
    assert len(inst) == len(rc.RS_CONFIGS)
    for k, (_, idx, elem) in enumerate(inst):
        assert (int(idx) if idx else len(inst) - 1) == k == int(elem)
    assert len(re.findall(r"switch \(cfg\)", api)) == 1
    for T, CPT, R, _ in rc.RS_CONFIGS:
        assert len(re.findall(r"<\s*%d\s*,\s*%d\s*,\s*%d\s*[,>]" % (T, CPT, R), re.sub(r"//[^\n]*", "", api))) == 1, (T, CPT, R)
    body = _body(api, r"void\s+launch_row_stream\s*\(\s*int\s+cfg\s*,")
    assert "with_rs_geom(cfg," in body and "launch_rs_mode<G>(mode, a, grid, s);" in body
    # the wide image is swept in panels above kMaxChunks, every panel with kPanelCfg; the Gram form stops at the same n
    assert "return H->nchunks > kMaxChunks;" in _body(api, r"bool\s+multi_panel\s*\(")
    assert re.search(r"H->ld\s*=\s*round_up\(std::max<int64_t>\(H->n,\s*1\),\s*16\);\s*H->nchunks\s*=\s*\(int\)\(H->ld\s*/\s*2\);", api)


def test_mirror_matches_grid_for_and_gram_geometry_in_the_source():
    """The two functions are compared as text (comments and layout aside): if either is edited, rs_cases.grid_for /
    rs_cases.gram_geometry have to be looked at again, and the expected text here updated with them."""
    api = _src("bh_api.hip")
    assert _body(api, r"int\s+grid_for\s*\(\s*int\s+cfg\s*,\s*int64_t\s+nrows\s*\)\s*\{") == (
        "const RsConfig& c = kRsConfigs[cfg]; const int64_t ngroups = (nrows + c.R - 1) / c.R; "
        "const int64_t bpc = g_ctx.opt_blocks_per_cu > 0 ? g_ctx.opt_blocks_per_cu : c.blocks_per_cu; "
        "int64_t g = (int64_t)g_ctx.n_cu * std::min<int64_t>(bpc, kMaxBlocksPerCu); "
        "g = std::min<int64_t>(g, std::max<int64_t>(ngroups, 1)); return (int)g;")
    assert _body(api, r"void\s+gram_geometry\s*\(") == (
        "const int64_t nrows = H->d + H->q_eff; "
        "const int64_t nb = (H->ld + GNG_BS - 1) / GNG_BS, nlb = nb * (nb + 1) / 2; int64_t s = 1; "
        "if (nlb < g_ctx.n_cu) s = std::max<int64_t>(1, std::min<int64_t>((2 * g_ctx.n_cu + nlb - 1) / nlb, (nrows + 255) / 256)); "
        "int64_t rows = round_up(std::max<int64_t>((nrows + s - 1) / s, 1), 16); s = std::max<int64_t>(1, (nrows + rows - 1) / rows); "
        "*nslabs = (int)s; *slab_rows = rows;")
    # spot values of the mirror itself
    assert rc.grid_for(6, 600, 256) == 256 and rc.grid_for(6, 100, 256) == 100 and rc.grid_for(0, 10 ** 6, 256, 0) == 2048
    assert rc.grid_for(rc.PANEL, 1100, 256, 0) == 256
    assert rc.gram_geometry(1000, 112, 256) == (4, 256) and rc.gram_geometry(100, 8192, 256) == (1, 112)


@pytest.mark.parametrize("n_cu", [256, 64, 304])
def test_cases_run_the_steady_state_loop_of_every_geometry(n_cu):
    cs = rc.cases(n_cu)
    assert len(set(cs)) == len(cs)
    for path in rc.PATHS:
        T, CPT, R, _ = rc.config_of(path)
        mine = [c for c in cs if c.path == path]
        assert mine, path
        lo, hi = rc.n_range(path)
        ns = sorted({c.n for c in mine})
        for c in mine:
            assert rc.path_of(c.n) == path and c.d > 0
        if path == rc.PANEL:
            # several launches per sweep, a different count of chunks in the narrow last one, t_out accumulated across them
            lasts = set()
            for n in ns:
                w = rc.panel_widths(n)
                assert len(w) >= 3 and w[-1] < rc.K_PANEL_CHUNKS and all(x == rc.K_PANEL_CHUNKS for x in w[:-1])
                lasts.add(w[-1])
            assert len(ns) >= 2 and len(lasts) >= 2
        else:
            assert hi in ns, "no n at the upper edge of geometry %r" % (path,)
        inside = [n for n in ns if n % 2 == 1 and lo < n and (hi is None or n < hi) and rc.ld_of(n) % (2 * T) != 0]
        assert inside, "no odd n strictly inside geometry %r with lanes idle in the last k" % (path,)
        shapes = [(c, rc.stream_shape(path, c.d + c.q, n_cu, 1)) for c in mine]
        for c, s in shapes:
            assert s["grid"] == n_cu, (c, s)                       # blocks_per_cu = 1 pins the grid
            if n_cu == 256:
                assert (c.d + c.q) * c.n <= (40e6 if path == rc.PANEL else 10.5e6), c

        def have(pred, what):
            hits = [c for c, s in shapes if pred(c, s)]
            assert hits, "geometry %r: no case with %s" % (path, what)
            return hits

        fulls = (True, False) if R > 1 else (True,)
        for full in fulls:
            tail_ok = (lambda s: s["tail"] == R) if full else (lambda s: 0 < s["tail"] < R)
            word = "a full" if full else "a partial"
            have(lambda c, s: s["passes"] >= 3 and s["passes"] % 2 == 1 and s["last_pass"] == s["passes"] and tail_ok(s),
                 ">= 3 passes ending on buffer A and %s last group" % word)
            have(lambda c, s: s["passes"] >= 2 and s["passes"] % 2 == 0 and s["last_pass"] == s["passes"] and tail_ok(s),
                 ">= 2 passes ending on buffer B and %s last group" % word)
            have(lambda c, s: s["ngroups"] == s["grid"] and tail_ok(s), "exactly `grid` row groups and %s last group" % word)
            have(lambda c, s: s["ngroups"] == s["grid"] + 1 and tail_ok(s), "grid + 1 row groups and %s last group" % word)
        # the multi-pass cases use both n
        assert {c.n for c, s in shapes if s["passes"] >= 2} == set(ns)
        # q >= 3 with the first mu row in a later pass — and, where a group has more than one row, inside a group
        hits = have(lambda c, s: c.q >= 3 and rc.mu_boundary(path, c.d, c.q, n_cu, 1)[0] >= 2, "q >= 3 and the mu boundary in a later pass")
        if R > 1:
            assert any(c.d % R != 0 for c in hits), "geometry %r: the mu boundary never falls inside a row group" % (path,)


@pytest.mark.parametrize("n_cu", [256, 64, 304])
def test_gram_cases_cover_the_slab_situations(n_cu):
    geo = {c: rc.gram_geometry(c.d + c.q, rc.ld_of(c.n), n_cu) for c in rc.GRAM_CASES}

    def first_estimates(c):
        nb = (rc.ld_of(c.n) + rc.GNG_BS - 1) // rc.GNG_BS
        nlb = nb * (nb + 1) // 2
        return nlb, (2 * n_cu + nlb - 1) // nlb, (c.d + c.q + 255) // 256

    def last(c):
        s, rows = geo[c]
        return c.d + c.q - (s - 1) * rows

    assert all(c.n <= 520 for c in rc.GRAM_CASES)
    assert any(s == 1 and c.d + c.q >= 16 for c, (s, rows) in geo.items())
    short = [c for c, (s, rows) in geo.items() if s > 1 and last(c) < rows]
    assert any(first_estimates(c)[2] < first_estimates(c)[1] for c in short), "no build whose slab count comes from (nrows + 255) / 256"
    assert any(first_estimates(c)[1] < first_estimates(c)[2] and first_estimates(c)[0] < n_cu for c in short), "no build limited by the CU count"
    assert any(c.d + c.q < 4 for c in geo) and any(4 <= c.d + c.q < 16 for c in geo)
    # one below / at / one above a slab boundary, all three with the same slab height
    trio = [(c, geo[c]) for c in rc.GRAM_CASES if "slab boundary" in c.why]
    assert len(trio) == 3 and len({rows for _, (s, rows) in trio}) == 1
    rows = trio[0][1][1]
    assert sorted((c.d + c.q) % rows for c, _ in trio) == [0, 1, rows - 1]
    assert sorted(last(c) for c, _ in trio) == [1, rows - 1, rows]
    # mu rows that start inside an MFMA k-step (4 rows) and in another slab than row 0
    assert any(c.q > 0 and c.d % 4 != 0 and c.d // geo[c][1] >= 1 for c in geo)
    mods = {c.n % 64 for c in rc.GRAM_CASES if c.n > 64}
    assert {63, 0, 1} <= mods
    assert any(c.n < 16 for c in rc.GRAM_CASES)
    w = rc.GRAM_WIDE_CASE
    assert 4096 < w.n <= 16384 and w.n % 2 == 1
