"""The option table (bh::Options, option_table, option_set, options_from_env of csrc/bh_options.h: no HIP in it) against the hand-written
lines it replaced.

A stand-alone program built by the host compiler (with the address and undefined-behaviour sanitizers) reads commands — set the 29
fields, one bh_set_option, one bh_init's worth of environment — and prints the return code, the fields and the detail text after each.

1. Parent equivalence.  `Parent` restates, arm by arm, bh_set_option (csrc/bh_api.hip:1535-1642 of the commit before the table) and the
   nine getenv lines of bh_init (:1472-1480), with the line of every arm.  It is written from that source, not from the table.
2. The table itself: unique keys, one key per field, every field reached, every default admissible.
3. The option list of include/benlsip_hip.h names exactly the table's keys, with the table's defaults and environment variables.
4. The wiring: bh_api.hip goes through the table and keeps the two keys that are no fields."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "benlsip.jl_amd", "csrc")

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
OK, INVALID_ARG, NOT_INIT = 0, -1, -2          # BH_OK, BH_ERR_INVALID_ARG, BH_ERR_NOT_INIT (include/benlsip_hip.h:44-46)
FOR_CALLER = 1                                   # kOptionForCaller: the arm stays in bh_api.hip
COERCE, CLAMP, REJECT, IGNORE, STORE, CALLER = range(6)          # enum OptionOutside

# struct Ctx, csrc/bh_api.hip:124-173 and :193 of the parent, in that order
FIELDS = ("opt_blocks_per_cu", "opt_batch", "opt_chol_downdate", "opt_cauchy_image", "opt_cauchy_image_max_ma", "opt_cauchy_image_refresh",
          "opt_cauchy_fused", "opt_cauchy_block", "opt_cauchy_gram_eq", "opt_cauchy_gram", "opt_linv_refine", "opt_cauchy_gemm",
          "opt_gram_cg_fused", "opt_gram_mfma", "opt_ls_from_cg", "opt_step_from_cg", "opt_fold_init", "opt_final_sync",
          "opt_host_copy_kernels", "opt_cg_fused", "opt_proj_form", "opt_upload_chunk_mb", "opt_free_image", "opt_free_image_minor",
          "opt_free_image_chain", "opt_free_image_eq", "opt_gram_ingest", "opt_ev_stride", "opt_image_pool")
# (`StepNotes notes`, :154, is no option.  29 fields, and 31 keys below: the numbers of the parent's source.)
DEFAULTS = dict(opt_blocks_per_cu=0, opt_batch=0, opt_chol_downdate=0, opt_cauchy_image=1, opt_cauchy_image_max_ma=64, opt_cauchy_image_refresh=0,
                opt_cauchy_fused=1, opt_cauchy_block=0, opt_cauchy_gram_eq=0, opt_cauchy_gram=0, opt_linv_refine=1, opt_cauchy_gemm=1,
                opt_gram_cg_fused=0, opt_gram_mfma=1, opt_ls_from_cg=1, opt_step_from_cg=0, opt_fold_init=1, opt_final_sync=0,
                opt_host_copy_kernels=1, opt_cg_fused=1, opt_proj_form=1, opt_upload_chunk_mb=64, opt_free_image=1, opt_free_image_minor=0,
                opt_free_image_chain=0, opt_free_image_eq=0, opt_gram_ingest=0, opt_ev_stride=8, opt_image_pool=2)
# every field at an admissible value that is not its default
OTHER = dict(opt_blocks_per_cu=3, opt_batch=5, opt_chol_downdate=1, opt_cauchy_image=0, opt_cauchy_image_max_ma=17, opt_cauchy_image_refresh=7,
             opt_cauchy_fused=0, opt_cauchy_block=4, opt_cauchy_gram_eq=1, opt_cauchy_gram=1, opt_linv_refine=0, opt_cauchy_gemm=0,
             opt_gram_cg_fused=1, opt_gram_mfma=2, opt_ls_from_cg=0, opt_step_from_cg=1, opt_fold_init=0, opt_final_sync=1,
             opt_host_copy_kernels=0, opt_cg_fused=2, opt_proj_form=0, opt_upload_chunk_mb=100, opt_free_image=2, opt_free_image_minor=1,
             opt_free_image_chain=1, opt_free_image_eq=1, opt_gram_ingest=1, opt_ev_stride=3, opt_image_pool=5)

KEYS = ("blocks_per_cu", "pcg_batch", "proj_form", "fold_init", "cg_fused", "final_sync", "host_copy_kernels", "ls_from_cg", "step_from_cg",
        "gram_mfma", "chol_downdate", "cauchy_image", "cauchy_gram", "cauchy_gram_eq", "gram_cg_fused", "cauchy_image_refresh", "cauchy_fused",
        "cauchy_block", "linv_refine", "cauchy_gemm", "cauchy_image_max_ma", "image_pool", "free_image", "free_image_minor", "free_image_chain",
        "free_image_eq", "gram_ingest", "upload_chunk_mb", "profile_stride", "comm_path", "profile")
NOT_KEYS = (None, "", "no_such_option", "free_image_", "cauchy")
VALUES = [INT64_MIN, -2, -1] + list(range(0, 18)) + [63, 64, 65, 96, 97, 4095, 4096, 4097, INT64_MAX]
ENV_NAMES = ("BH_HOST_COPY_KERNELS", "BH_BLOCKS_PER_CU", "BH_PCG_BATCH", "BH_PROJ_FORM", "BH_CG_FUSED", "BH_FINAL_SYNC", "BH_FREE_IMAGE",
             "BH_FREE_IMAGE_EQ", "BH_CAUCHY_BLOCK")
ENV_TEXTS = (None, "", "0", "1", "2", "3", "9", "-1", "16", "17", "abc", "2x")
# words, not numbers, in the header's brackets: the two keys that are no fields
WORD_DEFAULTS = ("comm_path", "profile")


def _max_blocks_per_cu():
    m = re.search(r"constexpr\s+int64_t\s+kMaxBlocksPerCu\s*=\s*(\d+)\s*;", open(os.path.join(CSRC, "bh_api.hip")).read())
    assert m
    return int(m.group(1))


K_MAX_BLOCKS_PER_CU = _max_blocks_per_cu()


# ---- the parent's lines, arm by arm (csrc/bh_api.hip of the commit before the table) ------------------------------------------------

def atoll(text):
    """strtoll(text, NULL, 10) on the texts used here: white space, a sign, digits; anything else ends the number; no digits: 0."""
    m = re.match(r"\s*([+-]?\d+)", text)
    return int(m.group(1)) if m else 0


def cauchy_block_value_ok(v):
    """csrc/bh_cauchy_plan.h:76."""
    return v in (0, 1, 2, 4, 8, 16)


class Parent:
    def __init__(self, fields, max_blocks_per_cu=K_MAX_BLOCKS_PER_CU):
        self.o = dict(fields)
        self.kMaxBlocksPerCu = max_blocks_per_cu                      # bh_api.hip:300

    def state(self):
        return tuple(self.o[f] for f in FIELDS)

    def set_option(self, key, value, init):
        """bh_set_option, bh_api.hip:1535-1642.  -> (code, detail); detail None where g_ctx.detail is not written."""
        o = self.o
        if key is None:                                               # :1536
            return INVALID_ARG, "NULL key"
        if key == "blocks_per_cu":                                    # :1537-1541
            if value < 0 or value > self.kMaxBlocksPerCu:
                return INVALID_ARG, "blocks_per_cu must be 0 (default) .. 8"
            o["opt_blocks_per_cu"] = value
            return OK, None
        if key == "pcg_batch":                                        # :1542
            o["opt_batch"] = max(0, value)
            return OK, None
        if key == "proj_form":                                        # :1543
            o["opt_proj_form"] = 1 if value else 0
            return OK, None
        if key == "fold_init":                                        # :1544
            o["opt_fold_init"] = 1 if value else 0
            return OK, None
        if key == "cg_fused":                                         # :1545-1549
            if value < 0 or value > 2:
                return INVALID_ARG, "cg_fused is 0, 1 (box constraints) or 2 (also linear equalities)"
            o["opt_cg_fused"] = value
            return OK, None
        if key == "final_sync":                                       # :1550
            o["opt_final_sync"] = 1 if value else 0
            return OK, None
        if key == "host_copy_kernels":                                # :1551
            o["opt_host_copy_kernels"] = 1 if value else 0
            return OK, None
        if key == "ls_from_cg":                                       # :1552
            o["opt_ls_from_cg"] = 1 if value else 0
            return OK, None
        if key == "step_from_cg":                                     # :1553
            o["opt_step_from_cg"] = 1 if value else 0
            return OK, None
        if key == "gram_mfma":                                        # :1554
            o["opt_gram_mfma"] = value
            return OK, None
        if key == "chol_downdate":                                    # :1555
            o["opt_chol_downdate"] = 1 if value else 0
            return OK, None
        if key == "cauchy_image":                                     # :1556
            o["opt_cauchy_image"] = 1 if value else 0
            return OK, None
        if key == "cauchy_gram":                                      # :1557
            o["opt_cauchy_gram"] = 1 if value else 0
            return OK, None
        if key == "cauchy_gram_eq":                                   # :1558-1562
            if value != 0 and value != 1:
                return INVALID_ARG, "cauchy_gram_eq is 0 or 1"
            o["opt_cauchy_gram_eq"] = value
            return OK, None
        if key == "gram_cg_fused":                                    # :1563-1569
            if value != 0 and not init:                               # :1565, BH_REQUIRE_INIT (:249-250)
                return NOT_INIT, "bh_init has not been called"
            if value != 0 and value != 1:                             # :1566
                return INVALID_ARG, "gram_cg_fused is 0 or 1"
            o["opt_gram_cg_fused"] = value
            return OK, None
        if key == "cauchy_image_refresh":                             # :1570-1574
            if value < 0:
                return INVALID_ARG, "cauchy_image_refresh is 0 (never) or the number of passes between two re-formations"
            o["opt_cauchy_image_refresh"] = value
            return OK, None
        if key == "cauchy_fused":                                     # :1575
            o["opt_cauchy_fused"] = 1 if value else 0
            return OK, None
        if key == "cauchy_block":                                     # :1576-1580
            if not cauchy_block_value_ok(value):
                return INVALID_ARG, "cauchy_block is 0, 1, 2, 4, 8 or 16 breakpoints per launch"
            o["opt_cauchy_block"] = value
            return OK, None
        if key == "linv_refine":                                      # :1581
            o["opt_linv_refine"] = 1 if value else 0
            return OK, None
        if key == "cauchy_gemm":                                      # :1582
            o["opt_cauchy_gemm"] = 1 if value else 0
            return OK, None
        if key == "cauchy_image_max_ma":                              # :1583
            o["opt_cauchy_image_max_ma"] = min(max(0, value), 64)
            return OK, None
        if key == "image_pool":                                       # :1584-1589 (the trim of the pool, :1587, is no field)
            if value < 0 or value > 8:
                return INVALID_ARG, "image_pool must be 0..8"
            o["opt_image_pool"] = value
            return OK, None
        if key == "free_image":                                       # :1590-1594
            if value < 0 or value > 2:
                return INVALID_ARG, "free_image is 0 (off), 1 (by the policy) or 2 (build at the first eligible call)"
            o["opt_free_image"] = value
            return OK, None
        if key == "free_image_minor":                                 # :1595-1599
            if value != 0 and value != 1:
                return INVALID_ARG, "free_image_minor is 0 or 1"
            o["opt_free_image_minor"] = value
            return OK, None
        if key == "free_image_chain":                                 # :1600-1604
            if value != 0 and value != 1:
                return INVALID_ARG, "free_image_chain is 0 or 1"
            o["opt_free_image_chain"] = value
            return OK, None
        if key == "free_image_eq":                                    # :1605-1609
            if value != 0 and value != 1:
                return INVALID_ARG, "free_image_eq is 0 or 1"
            o["opt_free_image_eq"] = value
            return OK, None
        if key == "gram_ingest":                                      # :1610-1614
            if value != 0 and value != 1:
                return INVALID_ARG, "gram_ingest is 0 or 1"
            o["opt_gram_ingest"] = value
            return OK, None
        if key == "upload_chunk_mb":                                  # :1615-1619
            if value < 1 or value > 4096:
                return INVALID_ARG, "upload_chunk_mb must be 1..4096"
            o["opt_upload_chunk_mb"] = value
            return OK, None
        if key == "profile_stride":                                   # :1620-1624
            if value < 1:
                return INVALID_ARG, "profile_stride must be >= 1"
            o["opt_ev_stride"] = value
            return OK, None
        if key == "comm_path":                                        # :1625-1639: communicator state, no opt_* field; stays in bh_api.hip
            return FOR_CALLER, None
        if key == "profile":                                          # :1640: g_ctx.flags, no opt_* field; stays in bh_api.hip
            return FOR_CALLER, None
        return INVALID_ARG, "unknown option " + key                   # :1641

    def init_env(self, env):
        """bh_init, bh_api.hip:1472-1480.  env: {name: text}; a name that is absent is a getenv that returns NULL."""
        o = self.o
        s = env.get("BH_HOST_COPY_KERNELS")                           # :1472
        if s is not None:
            o["opt_host_copy_kernels"] = 1 if atoll(s) else 0
        s = env.get("BH_BLOCKS_PER_CU")                               # :1473
        if s is not None:
            o["opt_blocks_per_cu"] = min(max(0, atoll(s)), self.kMaxBlocksPerCu)
        s = env.get("BH_PCG_BATCH")                                   # :1474
        if s is not None:
            o["opt_batch"] = max(0, atoll(s))
        s = env.get("BH_PROJ_FORM")                                   # :1475
        if s is not None:
            o["opt_proj_form"] = 1 if atoll(s) else 0
        s = env.get("BH_CG_FUSED")                                    # :1476
        if s is not None:
            o["opt_cg_fused"] = min(max(0, atoll(s)), 2)
        s = env.get("BH_FINAL_SYNC")                                  # :1477
        if s is not None:
            o["opt_final_sync"] = 1 if atoll(s) else 0
        s = env.get("BH_FREE_IMAGE")                                  # :1478
        if s is not None:
            o["opt_free_image"] = min(max(0, atoll(s)), 2)
        s = env.get("BH_FREE_IMAGE_EQ")                               # :1479
        if s is not None:
            o["opt_free_image_eq"] = 1 if atoll(s) != 0 else 0
        s = env.get("BH_CAUCHY_BLOCK")                                # :1480
        if s is not None:
            if cauchy_block_value_ok(atoll(s)):
                o["opt_cauchy_block"] = atoll(s)


# ---- the program ---------------------------------------------------------------------------------------------------------------------
# One command per line, fields separated by tabs:
#   D                     the defaults                      F v0 .. v28         the 29 fields
#   S key value init      option_set (@null: a NULL key)    E NAME=text ...     options_from_env; a name that is absent is not set
#   T                     the table, one line per row
# Every command but T answers `code <tab> the 29 fields <tab> text`: text is *why (S) or the names the environment was asked for (E).
PROGRAM = r"""
#include "bh_options.h"
#include <cstdio>
#include <iostream>
#include <map>
#include <sstream>
#include <vector>
using namespace bh;

#define FIELD_LIST(X) %s
#define AS_POINTER(f) &Options::f,
static constexpr int64_t Options::*kFields[] = {FIELD_LIST(AS_POINTER)};
constexpr int kNFields = (int)(sizeof(kFields) / sizeof(kFields[0]));
static_assert(sizeof(Options) == kNFields * sizeof(int64_t), "a field of Options is missing from the test's list");

int main(int argc, char** argv) {
    const int64_t max_bpc = argc > 1 ? std::atoll(argv[1]) : 0;
    Options o;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::vector<std::string> a;
        { std::stringstream ss(line); std::string t; while (std::getline(ss, t, '\t')) a.push_back(t); }
        if (line.size() && line.back() == '\t') a.push_back("");
        int32_t rc = 0;
        std::string text;
        if (a.empty()) continue;
        if (a[0] == "D") {
            o = Options();
        } else if (a[0] == "F") {
            if ((int)a.size() != 1 + kNFields) return 2;
            for (int i = 0; i < kNFields; ++i) o.*kFields[i] = std::stoll(a[1 + i]);
        } else if (a[0] == "S") {
            if (a.size() != 4) return 2;
            rc = option_set(o, a[1] == "@null" ? nullptr : a[1].c_str(), std::stoll(a[2]), a[3] == "1", &text, max_bpc);
        } else if (a[0] == "E") {
            std::map<std::string, std::string> env;
            for (size_t i = 1; i < a.size(); ++i) env[a[i].substr(0, a[i].find('='))] = a[i].substr(a[i].find('=') + 1);
            options_from_env(o, [&](const char* name) -> const char* {
                text += std::string(text.empty() ? "" : " ") + name;
                auto it = env.find(name);
                return it == env.end() ? nullptr : it->second.c_str();
            }, max_bpc);
        } else if (a[0] == "T") {
            const Options defaults;
            for (const OptionRow& r : option_table(max_bpc)) {
                int field = -1;
                for (int i = 0; i < kNFields; ++i) if (r.field != nullptr && r.field == kFields[i]) field = i;
                const long long def = r.field ? (long long)(defaults.*r.field) : 0;
                const bool def_ok = r.field ? (r.ok ? r.ok(def) : (def >= r.lo && def <= r.hi)) : true;
                std::printf("%%s\t%%d\t%%lld\t%%lld\t%%d\t%%s\t%%d\t%%d\t%%d\t%%lld\t%%d\t%%s\n", r.key, field, (long long)r.lo, (long long)r.hi, (int)r.outside,
                            r.env ? r.env : "-", (int)r.env_outside, r.ok ? 1 : 0, r.needs_init ? 1 : 0, def, def_ok ? 1 : 0, r.reject);
            }
            std::printf("END\n");
            continue;
        } else {
            return 3;
        }
        std::printf("%%d", (int)rc);
        for (int i = 0; i < kNFields; ++i) std::printf("\t%%lld", (long long)(o.*kFields[i]));
        std::printf("\t%%s\n", text.c_str());
    }
    return 0;
}
""" % " ".join("X(%s)" % f for f in FIELDS)


@pytest.fixture(scope="module")
def options_exe(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("options")
    src, exe = d / "options.cpp", d / "options"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    return str(exe)


def _state_command(fields):
    return "F\t" + "\t".join(str(fields[f]) for f in FIELDS)


def run_script(exe, commands):
    """-> per command (code, the 29 fields, text)."""
    out = subprocess.run([exe, str(K_MAX_BLOCKS_PER_CU)], input="\n".join(commands) + "\n", check=True, capture_output=True, text=True).stdout
    rows = []
    for ln in out.split("\n")[:-1]:
        parts = ln.split("\t")
        assert len(parts) == len(FIELDS) + 2, ln
        rows.append((int(parts[0]), tuple(int(x) for x in parts[1:-1]), parts[-1]))
    assert len(rows) == len(commands), (len(rows), len(commands))
    return rows


@pytest.fixture(scope="module")
def table(options_exe):
    out = subprocess.run([options_exe, str(K_MAX_BLOCKS_PER_CU)], input="T\n", check=True, capture_output=True, text=True).stdout.split("\n")
    assert out[-2:] == ["END", ""]
    names = ("key", "field", "lo", "hi", "outside", "env", "env_outside", "has_ok", "needs_init", "default", "default_ok", "reject")
    rows = []
    for ln in out[:-2]:
        r = dict(zip(names, ln.split("\t")))
        assert len(r) == len(names), ln
        rows.append({k: (v if k in ("key", "env", "reject") else int(v)) for k, v in r.items()})
    return rows


# ---- 1. parent equivalence ----------------------------------------------------------------------------------------------------------

def test_the_lists_of_this_file_are_whole():
    assert len(FIELDS) == 29 == len(set(FIELDS)) and set(DEFAULTS) == set(FIELDS) == set(OTHER)
    assert all(DEFAULTS[f] != OTHER[f] for f in FIELDS)
    assert len(KEYS) == 31 == len(set(KEYS)) and len(VALUES) == 30 and len(ENV_NAMES) == 9


def test_the_defaults_are_the_parents(options_exe):
    (rc, fields, text), = run_script(options_exe, ["D"])
    assert (rc, text) == (0, "") and dict(zip(FIELDS, fields)) == DEFAULTS


def test_set_option_equals_the_restated_arms(options_exe):
    cases, commands = [], []
    for start in (DEFAULTS, OTHER):
        for key in KEYS + NOT_KEYS:
            for init in (0, 1):
                for v in VALUES:
                    cases.append((start, key, v, init))
                    commands += [_state_command(start), "S\t%s\t%d\t%d" % ("@null" if key is None else key, v, init)]
    rows = run_script(options_exe, commands)
    for (start, key, v, init), (_, before, _), (rc, after, why) in zip(cases, rows[0::2], rows[1::2]):
        assert before == tuple(start[f] for f in FIELDS)
        p = Parent(start)
        want_rc, want_detail = p.set_option(key, v, bool(init))
        what = (key, v, init, "from the defaults" if start is DEFAULTS else "from the other state")
        assert rc == want_rc, what + (rc, want_rc)
        assert why == (want_detail or ""), what + (why, want_detail)
        assert after == p.state(), what + ([(f, a, b) for f, a, b in zip(FIELDS, after, p.state()) if a != b],)
        if rc != OK:
            assert after == before, what
    assert len(cases) == 2 * (len(KEYS) + 5) * 2 * len(VALUES)


def test_the_environment_equals_the_restated_lines(options_exe):
    envs = [{}]
    envs += [{name: text} for name in ENV_NAMES for text in ENV_TEXTS if text is not None]
    envs += [{name: text for name in ENV_NAMES} for text in ENV_TEXTS if text is not None]           # all nine set
    envs += [dict(zip(ENV_NAMES, ENV_TEXTS[1:10]))]
    # names the table does not know: other variables of the library, an option without a variable, a near miss
    strangers = {"BH_COMM": "ipc", "BH_FORCE_COMM": "1", "BH_FREE_IMAGE_MINOR": "1", "BH_CAUCHY_BLOCK_": "4", "bh_cg_fused": "0", "BH_GRAM_INGEST": "1"}
    envs += [strangers, dict(strangers, BH_CG_FUSED="0")]
    cases, commands = [], []
    for start in (DEFAULTS, OTHER):
        for env in envs:
            cases.append((start, env))
            commands += [_state_command(start), "\t".join(["E"] + ["%s=%s" % kv for kv in env.items()])]
    rows = run_script(options_exe, commands)
    for (start, env), (rc, after, asked) in zip(cases, rows[1::2]):
        p = Parent(start)
        p.init_env(env)
        assert rc == 0 and after == p.state(), (env, [(f, a, b) for f, a, b in zip(FIELDS, after, p.state()) if a != b])
        assert sorted(asked.split()) == sorted(ENV_NAMES), asked          # nine reads, each name once
        if env is strangers:
            assert after == tuple(start[f] for f in FIELDS)


def test_the_restatement_itself_on_values_known_from_the_header():
    """A few answers of `Parent` that include/benlsip_hip.h and the per-option tests state in words, so that the restatement is not the
    only witness of itself."""
    p = Parent(DEFAULTS)
    assert p.set_option("gram_cg_fused", 2, False) == (NOT_INIT, "bh_init has not been called")           # bh_init first, then the range
    assert p.set_option("gram_cg_fused", 2, True)[0] == INVALID_ARG and p.set_option("gram_cg_fused", 0, False) == (OK, None)
    assert p.set_option("blocks_per_cu", 9, True)[0] == INVALID_ARG and p.set_option("cauchy_block", 3, True)[0] == INVALID_ARG
    assert p.set_option("pcg_batch", -5, True) == (OK, None) and p.o["opt_batch"] == 0
    assert p.set_option("gram_mfma", 77, True) == (OK, None) and p.o["opt_gram_mfma"] == 77
    assert p.state() == tuple(dict(DEFAULTS, opt_gram_mfma=77)[f] for f in FIELDS)
    p.init_env({"BH_CG_FUSED": "9", "BH_FREE_IMAGE": "-1", "BH_CAUCHY_BLOCK": "3", "BH_BLOCKS_PER_CU": "17", "BH_PCG_BATCH": "2x"})
    assert (p.o["opt_cg_fused"], p.o["opt_free_image"], p.o["opt_cauchy_block"], p.o["opt_blocks_per_cu"], p.o["opt_batch"]) == (2, 0, 0, 8, 2)
    assert (atoll(""), atoll("abc"), atoll("2x"), atoll("-1"), atoll(" 17")) == (0, 0, 2, -1, 17)


# ---- 2. the table itself --------------------------------------------------------------------------------------------------------------

def test_the_table_has_one_row_per_key_and_one_key_per_field(table):
    keys = [r["key"] for r in table]
    assert len(keys) == len(set(keys)) == 31 and set(keys) == set(KEYS)
    stored = [r["field"] for r in table if r["outside"] != CALLER]
    assert all(0 <= f < len(FIELDS) for f in stored)
    assert len(stored) == len(set(stored))                            # no field has two keys
    assert set(stored) == set(range(len(FIELDS)))                     # ... and every field has one
    assert sorted(r["key"] for r in table if r["outside"] == CALLER) == sorted(WORD_DEFAULTS)
    assert all(r["field"] == -1 for r in table if r["outside"] == CALLER)


def test_every_default_is_admissible_and_every_rule_is_one_of_its_kind(table):
    for r in table:
        assert r["default_ok"] == 1, r
        assert r["lo"] <= r["hi"], r
        if r["outside"] == CALLER:
            continue
        assert r["default"] == DEFAULTS[FIELDS[r["field"]]], r
        assert r["outside"] in (COERCE, CLAMP, REJECT, STORE), r
        assert (r["reject"] != "") == (r["outside"] == REJECT), r     # a text exactly where a value can be refused
        if r["outside"] == COERCE or r["env_outside"] == COERCE and r["env"] != "-":
            assert (r["lo"], r["hi"]) == (0, 1), r
        if r["env"] != "-":
            assert r["env_outside"] in (COERCE, CLAMP, IGNORE), r
    assert sorted(r["env"] for r in table if r["env"] != "-") == sorted(ENV_NAMES)
    by = {r["key"]: r for r in table}
    assert by["blocks_per_cu"]["hi"] == K_MAX_BLOCKS_PER_CU          # the bound is the constant that sizes the slab buffers
    assert [r["key"] for r in table if r["needs_init"]] == ["gram_cg_fused"] and [r["key"] for r in table if r["has_ok"]] == ["cauchy_block"]


# ---- 3. the header -------------------------------------------------------------------------------------------------------------------

def _header_option_list():
    """-> {key: (the text in its brackets, its whole entry)} from the comment in front of bh_set_option."""
    hdr = open(os.path.join(ROOT, "include", "benlsip_hip.h")).read()
    i = hdr.index("int32_t bh_set_option(")
    text = hdr[hdr.rindex("/*", 0, i):i]
    heads = list(re.finditer(r'^ \*   "([a-z_]+)"', text, flags=re.M))
    out = {}
    for m, nxt in zip(heads, heads[1:] + [None]):
        entry = text[m.start():nxt.start() if nxt else len(text)]
        assert m.group(1) not in out, "two entries for %s" % m.group(1)
        b = re.match(r' \*   "[a-z_]+"\s*\[([^\]]*)\]', entry)
        assert b, "no [default] behind %s" % m.group(1)
        out[m.group(1)] = (b.group(1), entry)
    return out


def test_every_option_key_is_documented_in_the_header(table):
    """Every key of the table appears, quoted, in the option list of include/benlsip_hip.h — and the header documents no key the library
    does not know; the default in its brackets is the table's; the environment variable of a key is named in that key's entry."""
    documented = _header_option_list()
    accepted = {r["key"] for r in table}
    assert len(accepted) >= 15
    assert accepted - set(documented) == set(), "options without a line in the header: %s" % sorted(accepted - set(documented))
    assert set(documented) - accepted == set(), "header documents unknown options: %s" % sorted(set(documented) - accepted)
    for r in table:
        bracket, entry = documented[r["key"]]
        if r["key"] in WORD_DEFAULTS:
            assert not re.fullmatch(r"-?\d+", bracket), r["key"]
            continue
        assert re.fullmatch(r"-?\d+", bracket) and int(bracket) == r["default"], (r["key"], bracket, r["default"])
        if r["env"] != "-":
            assert re.search(r"\b%s\b" % r["env"], entry), "%s is not named in the entry of %s" % (r["env"], r["key"])
    for name in ENV_NAMES:                                             # ... and in no other key's entry
        assert [k for k, (_, entry) in documented.items() if re.search(r"\b%s\b" % name, entry)] == [r["key"] for r in table if r["env"] == name]


# ---- 4. the wiring -------------------------------------------------------------------------------------------------------------------

def test_the_host_file_goes_through_the_table():
    api = open(os.path.join(CSRC, "bh_api.hip")).read()
    header = open(os.path.join(CSRC, "bh_options.h")).read()
    assert '#include "bh_options.h"' in api
    assert re.findall(r'!strcmp\(key,\s*"([a-z_]+)"', api) == list(WORD_DEFAULTS)
    assert not re.search(r'strcmp\(\s*key', api.replace('!strcmp(key, "comm_path")', "").replace('!strcmp(key, "profile")', ""))
    for name in ENV_NAMES:
        assert name not in api, name
    for kept in ('getenv("BH_COMM")', 'getenv("BH_RCCL_LIB")', 'getenv("BH_FORCE_COMM")', 'getenv("BH_PEER_'):
        assert kept in api, kept
    assert api.count("options_from_env(g_ctx, getenv, kMaxBlocksPerCu);") == 1 and api.count("option_set(g_ctx, key, value, g_ctx.init, &why, kMaxBlocksPerCu)") == 1
    # bh_init: behind the allocations that can fail, in front of `init = true`, on the first initialisation only; bh_shutdown: no option
    body = api[api.index("int32_t bh_init(int32_t device, int32_t flags) {"):api.index("int32_t bh_shutdown(void) {")]
    assert body.index("BH_TRY(mbox_ensure());") < body.index("options_from_env(") < body.index("g_ctx.init = true;")
    assert body.index("if (g_ctx.init) {") < body.index("return BH_OK;") < body.index("options_from_env(")
    shutdown = api[api.index("int32_t bh_shutdown(void) {"):api.index("int32_t bh_set_stream(")]
    assert "opt_" not in shutdown and "Options" not in shutdown
    # the fields live in the header alone
    assert re.search(r"^struct Ctx : Options \{", api, flags=re.M) and not re.search(r"^\s*int64_t\s+opt_\w+\s*=", api, flags=re.M)
    assert re.findall(r"^\s*int64_t\s+(opt_\w+)\s*=", header, flags=re.M) == list(FIELDS)
    # ... which is plain C++: no HIP identifier, no HIP include
    code = re.sub(r"//[^\n]*", "", header)                          # (the fields' comments speak of hipEvents and of HIP)
    assert not re.search(r"\bhip\w*", code, flags=re.I), re.findall(r"\bhip\w*", code, flags=re.I)
    includes = re.findall(r"^\s*#\s*include\s*[<\"]([^>\"]+)[>\"]", header, flags=re.M)
    assert includes == ["../../include/benlsip_hip.h", "bh_cauchy_plan.h", "array", "cstdint", "cstdlib", "cstring", "string"], includes
    assert not re.search(r"\bstatic\b|\bextern\b|\bgetenv\b|\bstd::(cout|cerr|cin)\b|printf", header)          # no state, no I/O of its own
