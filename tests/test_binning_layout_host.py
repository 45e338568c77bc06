"""CPU test of the front end's buffer layouts (csrc/ggd_binning_layout.h): tests/host/binning_layout.cpp -- a stand-alone program
that includes nothing else -- is compiled with the system C++ compiler and -fsanitize=address,undefined and run as a child
process.  The expected numbers are the formulas of the code the header was lifted from (the parent commit's ggd_binning.hip,
ggd_rowbin.hip, ggd_rowbin_wide.inc and ggd_common.h), restated here; nothing is imported from the code under test."""
import itertools
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_gan_decoder_amd", "csrc")

PS = [1, 1024, 1025, 4096, 4097, 4096 * 256, 4096 * 256 + 1, 4096 * 257, 1_000_000]   # (256 / 257 tiles: the row count that once overflowed)
CAPS = [0, 1, 1024, 1025, 4_152_095]
GRIDS = [(16, 16), (1024, 1024), (1040, 1024), (1024, 1040), (4080, 4080)]          # 1x1, 64x64, 65x64, 64x65, 255x255 tiles
CASES = list(itertools.product(PS, CAPS, GRIDS))


# ---- the parent's formulas -----------------------------------------------------------------------------------------------
def align(v, a=256):
    return (v + a - 1) // a * a


def rs_gshift(n):                      # static inline int rs_gshift(int64_t ntiles)
    g = 2
    while (1 << (2 * g)) < n:
        g += 1
    return g


def rs_status_words(ntiles):           # (ntiles + (1 << rs_gshift(ntiles)) + 1) * RS_BINS
    return (ntiles + (1 << rs_gshift(ntiles)) + 1) * 256


RS_HWORDS, RS_MAX_PASSES = 8 * 256, 8
SORT_CTRL_BYTES = align((RS_HWORDS + 64) * 4)
FOLD_REPS, FOLD_REP_STRIDE = 16, 1024 + 256
FOLD_ROWTOT = FOLD_REPS * FOLD_REP_STRIDE + 64
FOLD_HEAD = FOLD_ROWTOT + FOLD_REPS * 64


def tiles(n, tile=4096):
    return max((n + tile - 1) // tile, 1)


def fold_l1_offset(P):
    return FOLD_HEAD + 4 * rs_status_words(tiles(P))


def fold_ctl_words(P):
    chunks = (P + 1023) // 1024
    return fold_l1_offset(P) + (chunks + (1 << rs_gshift(max(chunks, 1))) + 2) * 64


def rowbin(P, cap, W, H):
    """ggd_rowbin_tmp_bytes / the carving of ggd_launch_rowbin, narrow and wide"""
    gx, gy = (W + 15) // 16, (H + 15) // 16
    blocks1 = (P + 1023) // 1024
    if gx > 64 or gy > 64:
        nby, nbx = 64 * ((gy + 63) // 64), 64 * ((gx + 63) // 64)
        bins = 256
        tab_words = 2 * (bins + 1) + bins + bins + bins * bins          # RBW_TAB_WORDS
        blocks2 = ((cap + 1023) // 1024 + bins) & 0xffffffff
    else:
        nby = nbx = 64
        tab_words = 130 + 64 * 64 + 64 + 64                             # RB_TAB_WORDS
        blocks2 = ((cap + 1023) // 1024 + 64) & 0xffffffff
    sizes = [align(P * 8), align(blocks1 * nby * 4), align(tab_words * 4), align(cap * 8), align(blocks2 * nbx * 4)]
    offs = list(itertools.accumulate([0] + sizes))
    return dict(zip(("rb_packed", "rb_counts1", "rb_tab", "rb_ent", "rb_counts2", "rb_total"), offs))


def expected(P, cap, W, H):
    e = rowbin(P, cap, W, H)
    head = dict(ghist=0, tickets=RS_HWORDS, n_valid=RS_HWORDS + RS_MAX_PASSES, flat=RS_HWORDS + RS_MAX_PASSES + 1)
    for form in ("tmp", "clean"):      # ggd_sort32_nvalid_ptr / _flat_ptr; the status words at tmp + sort_ctrl_bytes() in both
        e.update({f"{form}_{k}": v for k, v in head.items()})
        e[f"{form}_status"], e[f"{form}_reps"] = SORT_CTRL_BYTES // 4, 1
    fh = FOLD_REPS * FOLD_REP_STRIDE   # ggd_fold_nvalid_ptr / _flat_ptr; status at fold->ctl + GGD_FOLD_HEAD
    e.update(fold_ghist=0, fold_tickets=fh, fold_n_valid=fh + RS_MAX_PASSES, fold_flat=fh + RS_MAX_PASSES + 1, fold_status=FOLD_HEAD,
             fold_reps=FOLD_REPS)
    nt = tiles(P)
    chunks = (P + 1023) // 1024
    e.update(pass1_status=rs_status_words(nt), rowtot=FOLD_ROWTOT, l1_status=fold_l1_offset(P),
             gshift_tiles=rs_gshift(nt), gshift_chunks=rs_gshift(max(chunks, 1)), status_words=rs_status_words(nt),
             fold_ctl_words=fold_ctl_words(P), fold_l1_offset=fold_l1_offset(P),
             sort_tmp_bytes=SORT_CTRL_BYTES + align(RS_MAX_PASSES * rs_status_words(nt) * 4),
             sort32_tmp_bytes=SORT_CTRL_BYTES + align(4 * rs_status_words(nt) * 4),
             msd_table_bytes=align(nt * 1024 * 4), ctrl_words=SORT_CTRL_BYTES // 4)
    return e


@pytest.fixture(scope="module")
def layouts(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and (shutil.which(c) or os.path.exists(c))), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("layout") / "binning_layout")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "host", "binning_layout.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], input="".join(f"{P} {cap} {W} {H}\n" for P, cap, (W, H) in CASES), capture_output=True, text=True,
                         timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    rows = [dict((kv.split("=")[0], kv.split("=")[1]) for kv in line.split()) for line in res.stdout.splitlines()]
    assert len(rows) == len(CASES)
    return rows


def test_header_includes_only_stdint_and_stddef():
    src = open(os.path.join(CSRC, "ggd_binning_layout.h")).read()
    assert [l.split()[1] for l in src.splitlines() if l.startswith("#include")] == ["<stdint.h>", "<stddef.h>"]


def test_every_figure_equals_the_parents_formula(layouts):
    for (P, cap, (W, H)), got in zip(CASES, layouts):
        want = expected(P, cap, W, H)
        assert got.pop("select") == "111", (P, cap, W, H)
        assert {k: int(v) for k, v in got.items()} == want, (P, cap, W, H)


def test_rowbin_total_is_the_end_of_the_last_region(layouts):
    for (P, cap, (W, H)), got in zip(CASES, layouts):
        wide = (W + 15) // 16 > 64 or (H + 15) // 16 > 64
        nbx = 64 * (((W + 15) // 16 + 63) // 64) if wide else 64
        blocks2 = (cap + 1023) // 1024 + (256 if wide else 64)
        assert int(got["rb_total"]) == int(got["rb_counts2"]) + align(blocks2 * nbx * 4), (P, cap, W, H)
        offs = [int(got[k]) for k in ("rb_packed", "rb_counts1", "rb_tab", "rb_ent", "rb_counts2", "rb_total")]
        assert offs == sorted(offs) and all(o % 256 == 0 for o in offs)


def test_the_257_tile_boundary_has_rows_for_every_group_choice(layouts):
    """257 launched tiles, 256 live ones: a pass may use 2^4 = 16 groups; the status rows must hold tiles + 16 (+ 1)"""
    by_p = {P: got for (P, cap, grid), got in zip(CASES, layouts)}
    assert int(by_p[4096 * 256]["gshift_tiles"]) == 4 and int(by_p[4096 * 257]["gshift_tiles"]) == 5
    assert int(by_p[4096 * 257]["status_words"]) // 256 - 257 >= 16 + 1
