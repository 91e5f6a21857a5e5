"""The three step-chain notes (bh::StepNotes, csrc/bh_step_chain_plan.h: no HIP in it) against the hand-written lines they replaced.

A stand-alone program built by the host compiler (with the address and undefined-behaviour sanitizers) reads a script — `S` sets the
three notes, every other command is one event or query — and prints the notes after each command, with what the command returned.
Pointers are symbolic: small integers cast to `const void*`, compared and never dereferenced.

1. Parent equivalence.  `Parent` restates, site by site, the 37 lines of csrc/bh_api.hip of the commit before the notes moved that set,
   compared or cleared `g_ctx.hw_note`, `g_ctx.hwc_note` and `g_ctx.gm_note` (line numbers of that file in every docstring).  For every
   site and every starting state of STATES the header's notes after the event equal the restated lines' — with ONE line of the
   restatement changed, bh_hess_set_mu, which now clears every note that names the handle as the other three handle sites do.  With
   that line as the parent had it the header disagrees at bh_hess_set_mu, exactly in the states where hw_note or gm_note names H, and
   at no other site that anything can observe.  (bh_shutdown: the parent left hw_note standing, the header clears it.  No call can
   tell: a match needs cg.hw != nullptr, the shutdown has dropped the workspace, and the next workspace is built through the
   slab-replaced site, which clears the note on either side.  The test shows that much instead of equality of the dead field.)

2. Sequences.  A chain step — bh_hmul_add_dev, bh_minor_iterate_dev, [a disturbance], bh_step_accumulate_dev, bh_model_reduction_dev —
   as its events, on the compact and on the full image, with the paths the rule gives (step_acc_select, model_select) restated from the
   event table of DESIGN.md §4.

3. The wiring: bh_api.hip speaks to the notes through the events alone."""
import itertools
import os
import re
import shutil
import subprocess

import pytest

from test_pcg_plan_cpu import CSRC

SWEEP, FULL, FULL_CARRY, COMPACT, COMPACT_CARRY = range(5)
MODEL_JV, MODEL_FROM_GMINOR, MODEL_CARRIED = range(3)

# the symbolic pointers
H, H2 = 1, 2
W, W2 = 11, 12
GM, GM2 = 21, 22
S, S2 = 31, 32
G, G2 = 41, 42
NF, NF2 = 100, 101

EVENTS = ("workspace_gone", "handle_changed", "compact_slots_changed", "cg_loop_begins", "compact_operands_overwritten", "minor_iterate_done",
          "gminor_written", "accumulate_begins", "accumulate_done", "model_query")

PROGRAM = r"""
#include "bh_step_chain_plan.h"
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <string>
using namespace bh;

static const void* P(long long v) { return reinterpret_cast<const void*>(static_cast<uintptr_t>(v)); }
static long long I(const void* p) { return static_cast<long long>(reinterpret_cast<uintptr_t>(p)); }

int main() {
    StepNotes n;
    std::string cmd;
    auto rd = [] { long long v = 0; std::cin >> v; return v; };
    while (std::cin >> cmd) {
        std::string res;
        auto add = [&](long long v) { res += " " + std::to_string(v); };
        if (cmd == "S") {
            n.full.H = P(rd()); n.full.w = P(rd()); n.full.gm = P(rd());
            n.compact.H = P(rd()); n.compact.w = P(rd()); n.compact.gm = P(rd()); n.compact.nfree = rd();
            n.gm.H = P(rd()); n.gm.s = P(rd()); n.gm.g = P(rd()); n.gm.gm = P(rd()); n.gm.fixed_part_stale = rd() != 0; n.gm.q_valid = rd() != 0;
        } else if (cmd == "workspace_gone") {
            n.workspace_gone();
        } else if (cmd == "handle_changed") {
            n.handle_changed(P(rd()));
        } else if (cmd == "compact_slots_changed") {
            n.compact_slots_changed(P(rd()));
        } else if (cmd == "cg_loop_begins") {
            n.cg_loop_begins(rd() != 0);
        } else if (cmd == "compact_operands_overwritten") {
            n.compact_operands_overwritten();
        } else if (cmd == "minor_iterate_done") {
            const void *h = P(rd()), *w = P(rd()), *gm = P(rd());
            const bool dev = rd() != 0, hw_kept = rd() != 0, compact = rd() != 0, chain = rd() != 0;
            n.minor_iterate_done(h, w, gm, dev, hw_kept, compact, chain, rd());
        } else if (cmd == "gminor_written") {
            const void *h = P(rd()), *s = P(rd()), *g = P(rd()), *gm = P(rd());
            n.gminor_written(h, s, g, gm, rd() != 0);
        } else if (cmd == "accumulate_begins" || cmd == "accumulate") {
            const void *h = P(rd()), *w = P(rd()), *gm = P(rd()), *s = P(rd()), *g = P(rd());
            const bool ok = rd() != 0, hw_live = rd() != 0, compact_live = rd() != 0;
            StepAccIn in = n.accumulate_begins(h, w, gm, s, g, ok, hw_live, compact_live, rd());
            add(in.full_note); add(in.compact_note); add(in.gm_note_match); add(in.fixed_part_stale); add(in.q_valid);
            if (cmd == "accumulate") {          // ... and the rest of bh_step_accumulate_dev: the options, the rule, the closing event
                in.step_from_cg = rd(); in.free_image_chain = rd();
                const StepAccPlan plan = step_acc_select(in);
                if (plan.path == STEP_ACC_SWEEP) n.gminor_written(h, s, g, gm, true);      // (through hmul_add_impl)
                else n.accumulate_done(h, s, g, gm, plan);
                add(plan.path); add(plan.q_init);
            }
        } else if (cmd == "accumulate_done") {
            const void *h = P(rd()), *s = P(rd()), *g = P(rd()), *gm = P(rd());
            StepAccPlan plan{};
            plan.fixed_part_stale = rd() != 0; plan.q_valid = rd() != 0;
            n.accumulate_done(h, s, g, gm, plan);
        } else if (cmd == "model_query" || cmd == "model") {
            const void *h = P(rd()), *s = P(rd()), *g = P(rd());
            const ModelQuery q = n.model_query(h, s, g);
            add(q.match); add(q.fixed_part_stale); add(q.q_valid); add(I(q.gm));
            if (cmd == "model") add(model_select(rd(), q.match, q.fixed_part_stale, q.q_valid));
        } else {
            std::printf("X unknown command %s\n", cmd.c_str());
            return 1;
        }
        std::printf("%lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %d %d |%s\n", I(n.full.H), I(n.full.w), I(n.full.gm), I(n.compact.H),
                    I(n.compact.w), I(n.compact.gm), (long long)n.compact.nfree, I(n.gm.H), I(n.gm.s), I(n.gm.g), I(n.gm.gm),
                    (int)n.gm.fixed_part_stale, (int)n.gm.q_valid, res.c_str());
    }
    return 0;
}
"""


@pytest.fixture(scope="module")
def notes_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("step_notes")
    src, exe = d / "notes.cpp", d / "notes"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


def run_script(exe, commands):
    """commands: tuples (name, ints...).  -> per command (notes as the 13-tuple of Parent.state(), the command's result as ints)."""
    text = "\n".join(" ".join(str(int(x)) if not isinstance(x, str) else x for x in c) for c in commands) + "\n"
    out = subprocess.run([exe], input=text, check=True, capture_output=True, text=True).stdout.splitlines()
    assert len(out) == len(commands), (len(out), len(commands), out[-1:])
    rows = []
    for line in out:
        st, res = line.split("|")
        rows.append((tuple(int(x) for x in st.split()), tuple(int(x) for x in res.split())))
    return rows


# ---- the parent's lines, site by site (csrc/bh_api.hip of the commit before the notes moved) -----------------------------------

class Parent:
    """g_ctx.hw_note {H, w, gm} (bh_api.hip:152), g_ctx.hwc_note {H, w, gm, nfree} (:176), g_ctx.gm_note {H, s, g, gm, fixed_part_stale,
    q_valid} (:156-157).  0 is nullptr; `= {}` is clear()."""

    def __init__(self, state, set_mu_as_on_the_parent=False):
        self.hw = dict(zip(("H", "w", "gm"), state[0:3]))
        self.hwc = dict(zip(("H", "w", "gm", "nfree"), state[3:7]))
        self.gmn = dict(zip(("H", "s", "g", "gm", "stale", "q"), state[7:13]))
        self.set_mu_as_on_the_parent = set_mu_as_on_the_parent

    def state(self):
        return tuple(self.hw.values()) + tuple(self.hwc.values()) + tuple(self.gmn.values())

    @staticmethod
    def clear(note):
        for k in note:
            note[k] = 0

    def slab_replaced(self):
        """ensure_cg_workspace, bh_api.hip:536-538."""
        self.clear(self.hw)                                          # :536
        self.clear(self.hwc)                                         # :537
        self.gmn["q"] = 0                                            # :538

    def shutdown(self):
        """bh_shutdown, bh_api.hip:1504-1505 (behind `c = CgWorkspace()`, :1503: cg.hw = nullptr, n_pad = 0)."""
        self.clear(self.hwc)                                         # :1504
        self.gmn["q"] = 0                                            # :1505

    def set_mu(self, h):
        """bh_hess_set_mu, bh_api.hip:2070-2071 (behind the early return for an unchanged mu, :2067).  THE ONE LINE THAT IS NOT THE
        PARENT'S: by default this site reads like the three below."""
        if not self.set_mu_as_on_the_parent:
            return self.set_form(h)
        if self.hwc["H"] == h:                                       # :2070
            self.clear(self.hwc)
        if self.gmn["H"] == h:                                       # :2071
            self.gmn["q"] = 0

    def gram_enter(self, h):
        """gram_enter, bh_api.hip:2098-2100."""
        if self.hw["H"] == h:                                        # :2098
            self.clear(self.hw)
        if self.hwc["H"] == h:                                       # :2099
            self.clear(self.hwc)
        if self.gmn["H"] == h:                                       # :2100
            self.clear(self.gmn)

    def set_form(self, h):
        """bh_hess_set_form, bh_api.hip:2120-2122."""
        if self.hw["H"] == h:                                        # :2120
            self.clear(self.hw)
        if self.hwc["H"] == h:                                       # :2121
            self.clear(self.hwc)
        if self.gmn["H"] == h:                                       # :2122
            self.clear(self.gmn)

    def destroy(self, h):
        """bh_hess_destroy, bh_api.hip:2177-2179 (in front of the NULL check, :2180)."""
        if h and self.hw["H"] == h:                                  # :2177
            self.clear(self.hw)
        if h and self.hwc["H"] == h:                                 # :2178
            self.clear(self.hwc)
        if h and self.gmn["H"] == h:                                 # :2179
            self.clear(self.gmn)

    def image_released(self, h):
        """free_image_release, bh_api.hip:2507."""
        if self.hwc["H"] == h:
            self.clear(self.hwc)

    def image_moved(self, h):
        """free_image_prepare, FI_MOVE, bh_api.hip:2551."""
        if self.hwc["H"] == h:
            self.clear(self.hwc)

    def image_built(self, h):
        """free_image_prepare, FI_BUILD, bh_api.hip:2574."""
        if self.hwc["H"] == h:
            self.clear(self.hwc)

    def pcg_run(self, hw_not_null):
        """pcg_run, bh_api.hip:2982-2983."""
        if hw_not_null:                                              # :2982
            self.clear(self.hw)
        self.clear(self.hwc)                                         # :2983

    def minor_iterate_host_staging(self):
        """minor_iterate_impl, `if (!dev)`, bh_api.hip:3244."""
        self.clear(self.hwc)

    def cauchy_host_staging(self):
        """cauchy_impl, `if (!dev)`, bh_api.hip:4020."""
        self.clear(self.hwc)

    def minor_iterate_end(self, h, w_out, g_model, dev, hw_not_null, fin_compact, chain, nfree):
        """minor_iterate_impl, bh_api.hip:3297, 3299."""
        if dev and hw_not_null and not fin_compact:                  # :3297
            self.hw["H"], self.hw["w"], self.hw["gm"] = h, w_out, g_model
        if dev and hw_not_null and fin_compact and chain:            # :3299
            self.hwc = dict(H=h, w=w_out, gm=g_model, nfree=nfree)

    def hmul_add_end(self, h, s_vec, g, out_n, dev):
        """hmul_add_impl, bh_api.hip:3383."""
        if dev:
            self.gmn = dict(H=h, s=s_vec, g=g, gm=out_n, stale=0, q=0)
        else:
            self.clear(self.gmn)

    def step_accumulate_begin(self, h, w_dev, gm_out, s_dev, g_dev, ok, c_hw, compact_live, nfree_now):
        """bh_step_accumulate_dev, bh_api.hip:3407-3414 (compact_live: `c.hwc != nullptr && H->fi.present && H->fi_map != nullptr`,
        nfree_now: H->fi.nfree).  -> (full_note, compact_note, gm_note_match, fixed_part_stale, q_valid)."""
        full = ok and self.hw["H"] == h and self.hw["w"] == w_dev and self.hw["gm"] == gm_out and c_hw                            # :3407
        compact = (ok and self.hwc["H"] == h and self.hwc["w"] == w_dev and self.hwc["gm"] == gm_out and compact_live and
                   nfree_now == self.hwc["nfree"])                                                                                # :3408-3409
        match = ok and self.gmn["H"] == h and self.gmn["s"] == s_dev and self.gmn["g"] == g_dev and self.gmn["gm"] == gm_out        # :3410
        flags = (self.gmn["stale"], self.gmn["q"])                                                                                # :3411
        self.clear(self.hw)                                          # :3413
        self.clear(self.hwc)                                         # :3414
        return (int(bool(full)), int(bool(compact)), int(bool(match))) + flags

    def step_accumulate_end(self, h, s_dev, g_dev, gm_out, plan_stale, plan_q):
        """bh_step_accumulate_dev, bh_api.hip:3436."""
        self.gmn = dict(H=h, s=s_dev, g=g_dev, gm=gm_out, stale=plan_stale, q=plan_q)

    def model_reduction(self, h, s_dev, g_dev):
        """bh_model_reduction_dev, bh_api.hip:3531-3532, 3544: -> (note, the two flags as model_select got them, the pointer the
        kernel was given)."""
        note = self.gmn["H"] == h and self.gmn["s"] == s_dev and self.gmn["g"] == g_dev and self.gmn["gm"] != 0                  # :3531
        return (int(note), self.gmn["stale"], self.gmn["q"], self.gmn["gm"])                                                      # :3532, :3544


def _states():
    """Each note empty, naming H (and the call's other pointers, or one of them not), naming another handle; every flag combination."""
    full = [(0, 0, 0), (H, W, GM), (H2, W, GM), (H, W2, GM), (H, W, GM2)]
    compact = [(0, 0, 0, 0), (H, W, GM, NF), (H2, W, GM, NF), (H, W2, GM, NF), (H, W, GM2, NF), (H, W, GM, NF2)]
    gm = [(0, 0, 0, 0), (H, S, G, GM), (H2, S, G, GM), (H, S2, G, GM), (H, S, G2, GM), (H, S, G, GM2), (H, S, G, 0)]
    flags = list(itertools.product((0, 1), repeat=2))
    return [f + c + g + fl for f, c, g, fl in itertools.product(full, compact, gm, flags)]


STATES = _states()
B2 = list(itertools.product((0, 1), repeat=2))
B4 = list(itertools.product((0, 1), repeat=4))

# site -> [(the header's event as a command, the site's call on Parent as (method, args))]
SITES = {
    "slab_replaced": [(("workspace_gone",), ("slab_replaced", ()))],
    "shutdown": [(("workspace_gone",), ("shutdown", ()))],
    "set_mu": [(("handle_changed", h), ("set_mu", (h,))) for h in (H, H2)],
    "gram_enter": [(("handle_changed", h), ("gram_enter", (h,))) for h in (H, H2)],
    "set_form": [(("handle_changed", h), ("set_form", (h,))) for h in (H, H2)],
    "destroy": [(("handle_changed", h), ("destroy", (h,))) for h in (H, H2, 0)],
    "image_released": [(("compact_slots_changed", h), ("image_released", (h,))) for h in (H, H2)],
    "image_moved": [(("compact_slots_changed", h), ("image_moved", (h,))) for h in (H, H2)],
    "image_built": [(("compact_slots_changed", h), ("image_built", (h,))) for h in (H, H2)],
    "pcg_run": [(("cg_loop_begins", b), ("pcg_run", (b,))) for b in (0, 1)],
    "minor_iterate_host_staging": [(("compact_operands_overwritten",), ("minor_iterate_host_staging", ()))],
    "cauchy_host_staging": [(("compact_operands_overwritten",), ("cauchy_host_staging", ()))],
    "minor_iterate_end": [(("minor_iterate_done", H, W, GM) + b + (NF,), ("minor_iterate_end", (H, W, GM) + b + (NF,))) for b in B4],
    "hmul_add_end": [(("gminor_written", H, S, G, GM, dev), ("hmul_add_end", (H, S, G, GM, dev))) for dev in (0, 1)],
    "step_accumulate_begin": [(("accumulate_begins", H, W, GM, S, G) + b[:3] + (NF2 if b[3] else NF,),
                               ("step_accumulate_begin", (H, W, GM, S, G) + b[:3] + (NF2 if b[3] else NF,))) for b in B4],
    "step_accumulate_end": [(("accumulate_done", H, S, G, GM) + b, ("step_accumulate_end", (H, S, G, GM) + b)) for b in B2],
    "model_reduction": [(("model_query", H, S, G), ("model_reduction", (H, S, G)))],
}


@pytest.fixture(scope="module")
def header_after(notes_exe):
    """(site, index of the call at that site, starting state) -> (the header's notes afterwards, what the event returned)."""
    keys, commands = [], []
    for site, calls in SITES.items():
        for i, (event, _) in enumerate(calls):
            for st in STATES:
                keys.append((site, i, st))
                commands += [("S",) + st, event]
    rows = run_script(notes_exe, commands)
    for k, (st, _) in zip(keys, rows[0::2]):
        assert st == k[2], ("S did not set the state", k, st)
    return dict(zip(keys, rows[1::2]))


def _parent_after(site, i, st, **kw):
    p = Parent(st, **kw)
    method, args = SITES[site][i][1]
    res = getattr(p, method)(*args)
    return p.state(), (tuple(res) if res is not None else ())


def test_every_site_names_an_event_and_every_event_has_a_site(header_after):
    assert {calls[0][0][0] for calls in SITES.values()} == set(EVENTS)
    assert len(STATES) == 5 * 6 * 7 * 4 and len(set(STATES)) == len(STATES)
    assert len(header_after) == len(STATES) * sum(len(c) for c in SITES.values())


def test_the_header_equals_the_restated_lines_at_every_site(header_after):
    for (site, i, st), (got_state, got_res) in header_after.items():
        if site == "shutdown":
            continue                                                  # (the test below)
        want_state, want_res = _parent_after(site, i, st)
        assert got_state == want_state, (site, SITES[site][i][0], st, got_state, want_state)
        assert got_res == want_res, (site, SITES[site][i][0], st, got_res, want_res)


def test_set_mu_is_the_only_site_where_the_parent_did_otherwise(header_after):
    differ = 0
    for (site, i, st), (got_state, got_res) in header_after.items():
        if site == "shutdown":
            continue
        want_state, want_res = _parent_after(site, i, st, set_mu_as_on_the_parent=True)
        if site != "set_mu":
            assert (got_state, got_res) == (want_state, want_res), (site, st)
            continue
        h = SITES[site][i][1][1][0]
        names = st[0] == h or st[7] == h                            # hw_note or gm_note names the handle whose mu changes
        assert (got_state != want_state) == names, (h, st, got_state, want_state)
        if names:
            differ += 1
            # the parent kept what the header drops: cg.hw's note as it was, gm_note with q_valid cleared and nothing else
            assert want_state[0:3] == st[0:3] and want_state[7:12] == st[7:12] and want_state[12] == (0 if st[7] == h else st[12])
            assert got_state[0:3] == ((0, 0, 0) if st[0] == h else st[0:3]) and got_state[7:13] == ((0,) * 6 if st[7] == h else st[7:13])
        assert got_state[3:7] == want_state[3:7]                    # the compact note fell on the parent too
    assert differ > 0


def test_shutdown_differs_from_the_parent_in_a_note_nothing_can_read(header_after, notes_exe):
    """bh_api.hip:1503-1505 left hw_note standing.  Until the next workspace exists cg.hw is null (hw_live = 0): the accumulate gets the
    same answers and leaves the same notes; and that workspace comes through the slab-replaced site (n_pad = 0 < any n_pad)."""
    commands, wants = [], []
    for (site, i, st), (got_state, got_res) in header_after.items():
        if site != "shutdown":
            continue
        want_state, _ = _parent_after(site, i, st)
        assert got_state[3:] == want_state[3:], st
        assert got_state[0:3] == (0, 0, 0) and want_state[0:3] == st[0:3]
        for ok, compact_live in B2:
            p = Parent(want_state)
            res = p.step_accumulate_begin(H, W, GM, S, G, ok, 0, compact_live, NF)
            commands += [("S",) + got_state, ("accumulate_begins", H, W, GM, S, G, ok, 0, compact_live, NF)]
            wants.append((p.state(), res))
        p = Parent(want_state)
        p.slab_replaced()
        commands += [("S",) + got_state, ("workspace_gone",)]
        wants.append((p.state(), ()))
    rows = run_script(notes_exe, commands)[1::2]
    assert len(wants) == 5 * len(STATES)
    for got, want in zip(rows, wants):
        assert got == want, (got, want)


# ---- sequences ---------------------------------------------------------------------------------------------------------------------
# What lies between the minor iterate and the accumulate, as the events bh_api.hip raises (h: the handle the disturbance is about),
# and the accumulate's path behind it on the compact and on the full image when h is the chain's handle, from the event table:
#   cg_loop_begins(writes_hw)       full := {} if writes_hw; compact := {}
#   handle_changed(h)               every note that names h := {}
#   workspace_gone                  full := {}; compact := {}; gm.q_valid := false
#   compact_slots_changed(h)        compact := {} if it names h
#   compact_operands_overwritten    compact := {}
DISTURBANCES = {
    # bh_pcg_dev: a loop that accumulates no H*w — cg.hw stays what it was
    "pcg": (lambda h: [("cg_loop_begins", 0)], SWEEP, FULL),
    # a bh_minor_iterate_dev on another handle: always "other" (below)
    "set_mu": (lambda h: [("handle_changed", h)], SWEEP, SWEEP),
    "set_form": (lambda h: [("handle_changed", h)], SWEEP, SWEEP),
    "destroy": (lambda h: [("handle_changed", h)], SWEEP, SWEEP),
    "slab_replaced": (lambda h: [("workspace_gone",)], SWEEP, SWEEP),
    "image_moved": (lambda h: [("compact_slots_changed", h)], SWEEP, FULL),
    # FI_BUILD: free_image_release, then the build
    "image_built_again": (lambda h: [("compact_slots_changed", h), ("compact_slots_changed", h)], SWEEP, FULL),
    # bh_minor_iterate (ls_from_cg = 1): staging, the loop with H*w, and a host-pointer call notes nothing
    "host_minor_iterate": (lambda h: [("compact_operands_overwritten",), ("cg_loop_begins", 1), ("minor_iterate_done", h, W2, GM2, 0, 1, 0, 0, NF)],
                           SWEEP, SWEEP),
    "host_cauchy_step": (lambda h: [("compact_operands_overwritten",)], SWEEP, FULL),
}
# cleared whatever handle the call is about
REGARDLESS = {"pcg", "slab_replaced", "host_minor_iterate", "host_cauchy_step"}
UNDISTURBED = {True: COMPACT_CARRY, False: FULL}


def _chain_head(compact):
    """bh_hmul_add_dev(H, s, g, gm); bh_minor_iterate_dev(H, ..., g_model = gm, w) under step_from_cg = 1 [free_image_chain = 1]."""
    return [("gminor_written", H, S, G, GM, 1), ("cg_loop_begins", 1), ("minor_iterate_done", H, W, GM, 1, 1, int(compact), int(compact), NF)]


def _accumulate(compact, w=W):
    return ("accumulate", H, w, GM, S, G, 1, 1, 1, NF, 1, int(compact))


def _paths(exe, commands):
    """-> the paths of the `accumulate` and `model` commands, in order, and whether each accumulate initialised q."""
    rows = run_script(exe, commands)
    acc = [(r[1][5], r[1][6]) for c, r in zip(commands, rows) if c[0] == "accumulate"]
    mod = [r[1][4] for c, r in zip(commands, rows) if c[0] == "model"]
    return acc, mod, rows


MODEL = ("model", H, S, G, 1)


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "full"])
def test_an_undisturbed_step_and_the_four_disturbances_of_the_gpu_test(notes_exe, compact):
    """pcg, other_handle, other_w, second_accumulate of
    test_free_image_chain_gpu.py::test_anything_between_the_minor_iterate_and_the_accumulate_sends_it_down_the_sweep."""
    head = _chain_head(compact)
    acc, mod, _ = _paths(notes_exe, head + [_accumulate(compact), MODEL])
    assert acc == [(UNDISTURBED[compact], int(compact))]           # the compact chain has no q yet: q0 from the whole g_minor first
    assert mod == [MODEL_CARRIED if compact else MODEL_FROM_GMINOR]
    # pcg: the compact operands are gone; cg.hw is not (full image: the two vector launches stay right)
    acc, mod, _ = _paths(notes_exe, head + DISTURBANCES["pcg"][0](H) + [_accumulate(compact), MODEL])
    assert acc == [(SWEEP if compact else FULL, 0)] and mod == [MODEL_FROM_GMINOR]
    # other_handle: a minor iterate on H2 has run its loop and noted its own w
    other = [("cg_loop_begins", 1), ("minor_iterate_done", H2, W2, GM2, 1, 1, int(compact), int(compact), NF2)]
    acc, mod, _ = _paths(notes_exe, head + other + [_accumulate(compact), MODEL])
    assert acc == [(SWEEP, 0)] and mod == [MODEL_FROM_GMINOR]
    # other_w: a copy of w at another address
    acc, mod, _ = _paths(notes_exe, head + [_accumulate(compact, w=W2), MODEL])
    assert acc == [(SWEEP, 0)] and mod == [MODEL_FROM_GMINOR]
    # second_accumulate: one use
    acc, mod, rows = _paths(notes_exe, head + [_accumulate(compact), _accumulate(compact), MODEL])
    assert acc == [(UNDISTURBED[compact], int(compact)), (SWEEP, 0)] and mod == [MODEL_FROM_GMINOR]
    assert rows[-1][0][11:13] == (0, 0)                             # the sweep rewrote all of g_minor: both flags fell


@pytest.mark.parametrize("compact", [True, False], ids=["compact", "full"])
@pytest.mark.parametrize("name", list(DISTURBANCES))
def test_a_disturbance_on_the_handle_and_on_another(notes_exe, name, compact):
    events, on_compact, on_full = DISTURBANCES[name]
    head = _chain_head(compact)
    acc, mod, rows = _paths(notes_exe, head + events(H) + [_accumulate(compact), MODEL])
    want = on_compact if compact else on_full
    assert acc == [(want, 0)], (name, acc)
    assert mod == [MODEL_FROM_GMINOR], (name, mod)                   # a sweep, or the full image's two launches: g_minor is whole
    assert rows[-1][0][7:13] == (H, S, G, GM, 0, 0)
    # the same call about another handle
    acc, mod, _ = _paths(notes_exe, head + events(H2) + [_accumulate(compact), MODEL])
    want = (on_compact if compact else on_full) if name in REGARDLESS else UNDISTURBED[compact]
    assert acc == [(want, int(compact and want == COMPACT_CARRY))], (name, "other handle", acc)
    assert mod == [MODEL_CARRIED if want == COMPACT_CARRY else MODEL_FROM_GMINOR], (name, "other handle", mod)


def test_what_becomes_of_the_model_value(notes_exe):
    head = _chain_head(True)
    # bh_hmul_add_dev, another mu, bh_model_reduction_dev: g_minor is of the old operator — the J v sweep
    _, mod, _ = _paths(notes_exe, [("gminor_written", H, S, G, GM, 1), MODEL, ("handle_changed", H), MODEL])
    assert mod == [MODEL_FROM_GMINOR, MODEL_JV]
    # ... of another handle: nothing happens
    _, mod, _ = _paths(notes_exe, [("gminor_written", H, S, G, GM, 1), ("handle_changed", H2), MODEL])
    assert mod == [MODEL_FROM_GMINOR]
    # a carried q goes with the workspace, and the stale g_minor it stood in for is not used: the J v sweep
    acc, mod, rows = _paths(notes_exe, head + [_accumulate(True), MODEL, ("workspace_gone",), MODEL])
    assert acc == [(COMPACT_CARRY, 1)] and mod == [MODEL_CARRIED, MODEL_JV]
    assert rows[-1][0][7:13] == (H, S, G, GM, 1, 0)
    # two compact steps: the second one carries the q of the first (no q_init); then a full-image step carries it on
    second = [("cg_loop_begins", 1), ("minor_iterate_done", H, W, GM, 1, 1, 1, 1, NF)]
    third = [("cg_loop_begins", 1), ("minor_iterate_done", H, W, GM, 1, 1, 0, 1, NF)]
    acc, mod, rows = _paths(notes_exe, head + [_accumulate(True)] + second + [_accumulate(True)] + third + [_accumulate(True), MODEL])
    assert acc == [(COMPACT_CARRY, 1), (COMPACT_CARRY, 0), (FULL_CARRY, 0)] and mod == [MODEL_CARRIED]
    assert rows[-1][0][7:13] == (H, S, G, GM, 1, 1)
    # a host-pointer bh_hmul_add writes no device g_minor: the note falls, flags included
    _, mod, rows = _paths(notes_exe, head + [_accumulate(True), ("gminor_written", H, S, G, GM, 0), MODEL])
    assert mod == [MODEL_JV] and rows[-1][0][7:13] == (0,) * 6
    # the image has another width than the one noted: not this call's cg.hwc
    acc, _, _ = _paths(notes_exe, head + [("accumulate", H, W, GM, S, G, 1, 1, 1, NF2, 1, 1)])
    assert acc == [(SWEEP, 0)]


# ---- the wiring --------------------------------------------------------------------------------------------------------------------
def test_the_host_file_speaks_to_the_notes_through_the_events_alone():
    api = open(os.path.join(CSRC, "bh_api.hip")).read()
    header = open(os.path.join(CSRC, "bh_step_chain_plan.h")).read()
    assert '#include "bh_step_chain_plan.h"' in api
    for old in ("hw_note", "hwc_note", "gm_note"):
        assert old not in api, old
    assert len(re.findall(r"^\s*StepNotes notes;", api, flags=re.M)) == 1
    uses = re.findall(r"\bnotes\s*(?:\.|->)\s*(\w+)\s*(\(?)", api)
    assert uses and all(name in EVENTS and paren == "(" for name, paren in uses), [u for u in uses if u[0] not in EVENTS or u[1] != "("]
    assert {name for name, _ in uses} == set(EVENTS)
    assert len(re.findall(r"\bnotes\b", api)) == len(uses) + 1      # (every mention is the member or a call on it)
    # the sites of the handle event: mu, into and out of the Gram form, destroy
    def body_of(fn):
        found = re.findall(r"^[\w ]*\b%s\(bh_hess\* H[^)]*\) \{\n(.*?)\n\}\n" % fn, api, flags=re.M | re.S)
        assert len(found) == 1, fn
        return found[0]
    for fn in ("bh_hess_set_mu", "gram_enter", "bh_hess_set_form", "bh_hess_destroy"):
        assert body_of(fn).count("g_ctx.notes.handle_changed(H);") == 1, fn
    body = body_of("bh_hess_set_mu")
    assert body.index("if (mu == H->mu) return BH_OK;") < body.index("handle_changed")      # an unchanged mu costs nothing
    body = body_of("bh_hess_destroy")
    assert body.index("handle_changed") < body.index("if (!H) return BH_OK;")
    # the header: plain values only
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", header, flags=re.M)
    assert includes == ["cstdint"], includes
    for name in EVENTS:
        assert re.search(r"\b%s\(" % name, header), name
