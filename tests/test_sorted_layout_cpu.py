"""The workspace layout of the two sorted forms of the Cauchy search (csrc/bh_cauchy_sort_layout.h: cauchy_sort_layout, the one
statement that the allocation, the memset of the hand-back flag and the launcher of bh_api.hip read): a stand-alone program built by
the host compiler prints the offsets for both forms; they are compared with the numbers written out here."""
import os
import shutil
import subprocess

import pytest

import test_cauchy_plan_cpu as base

LDS, GRIDS = (16, 32, 4096, 16384), (1, 256)
PROGRAM = r"""
#include "bh_cauchy_sort_layout.h"
#include <cstdio>
int main() {
    const long long lds[] = {%s};
    const int grids[] = {%s};
    for (long long ld : lds) for (int form = 5; form <= 6; ++form) for (int grid : grids) {
        if (form == 5 && grid != grids[0]) continue;
        const bh::CauchySortLayout o = bh::cauchy_sort_layout(ld, (bh::CauchyForm)form, grid);
        std::printf("%%lld %%d %%d %%lld %%lld %%lld %%lld %%lld %%lld %%lld %%lld %%lld %%lld %%lld\n", ld, form, grid, (long long)o.T, (long long)o.b,
                    (long long)o.UL, (long long)o.red, (long long)o.scan, (long long)o.rank, (long long)o.inv, (long long)o.flag, (long long)o.head,
                    (long long)o.slab, (long long)o.total);
    }
    return 0;
}
""" % (", ".join(str(v) for v in LDS), ", ".join(str(v) for v in GRIDS))
FIELDS = ("T", "b", "UL", "red", "scan", "rank", "inv", "flag", "head", "slab", "total")
TABLE = {                       # (ld, form, grid): the offsets in doubles, in the order of FIELDS (-1: no such region)
    (16, 5, 1): (0, 16, 32, -1, 160, 256, 264, 272, 288, -1, 288),
    (16, 6, 1): (0, 16, -1, 32, 64, 96, 104, 112, 128, 128, 160),
    (16, 6, 256): (0, 16, -1, 32, 64, 96, 104, 112, 128, 128, 8320),
    (32, 5, 1): (0, 32, 64, -1, 320, 464, 480, 496, 512, -1, 512),
    (32, 6, 1): (0, 32, -1, 64, 128, 176, 192, 208, 224, 224, 288),
    (32, 6, 256): (0, 32, -1, 64, 128, 176, 192, 208, 224, 224, 16608),
    (4096, 5, 1): (0, 4096, 8192, -1, 40960, 53296, 55344, 57392, 57408, -1, 57408),
    (4096, 6, 1): (0, 4096, -1, 8192, 16384, 20496, 22544, 24592, 24608, 24608, 32800),
    (4096, 6, 256): (0, 4096, -1, 8192, 16384, 20496, 22544, 24592, 24608, 24608, 2121760),
    (16384, 5, 1): (0, 16384, 32768, -1, 163840, 213040, 221232, 229424, 229440, -1, 229440),
    (16384, 6, 1): (0, 16384, -1, 32768, 65536, 81936, 90128, 98320, 98336, 98336, 131104),
    (16384, 6, 256): (0, 16384, -1, 32768, 65536, 81936, 90128, 98320, 98336, 98336, 8486944),
}


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    d = tmp_path_factory.mktemp("sorted_layout")
    src, exe = d / "layout.cpp", d / "layout"
    src.write_text(PROGRAM)
    subprocess.run([cxx, "-std=c++17", "-Wall", "-Werror", "-I", base.CSRC, str(src), "-o", str(exe)], check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()
    rows = [tuple(int(x) for x in ln.split()) for ln in out]
    return {r[:3]: dict(zip(FIELDS, r[3:])) for r in rows}


def test_offsets_are_the_table(layouts):
    """Form 5: T 0, b ld, UL 2 ld (8 ld doubles), scan 10 ld (3 (ld + 16)), rank 13 ld + 48, flag 14 ld + 48, total 14 ld + 64.
    Form 6: T 0, b ld, red 2 ld (2 ld doubles), scan 4 ld (ld + 16), rank 5 ld + 16, flag 6 ld + 16, head 6 ld + 32, then the slabs."""
    assert sorted(layouts) == sorted(TABLE)
    for key, want in TABLE.items():
        assert layouts[key] == dict(zip(FIELDS, want)), (key, layouts[key], want)


def test_regions_are_ordered_disjoint_even_and_inside(layouts):
    """The regions in the order of the table, each ending where the next begins or before it; every offset even (b and rank are read
    as 16- and 8-byte vectors); the flag inside the allocation."""
    for (ld, form, grid), o in layouts.items():
        mid, mid_len, nscan = ("UL", 8 * ld, 3) if form == 5 else ("red", 2 * ld, 1)
        regions = [("T", ld), ("b", ld), (mid, mid_len), ("scan", nscan * (ld + 16)), ("rank", ld // 2), ("inv", ld // 2), ("flag", 1)]
        if form == 6:
            regions.append(("slab", grid * 2 * ld))
        end = 0
        for name, length in regions:
            assert o[name] >= end and o[name] % 2 == 0, (ld, form, grid, name, o)
            end = o[name] + length
        assert end <= o["total"] and o["flag"] + 1 <= o["head"] <= o["total"], (ld, form, grid, o)
        assert o["UL" if form == 6 else "red"] == -1
