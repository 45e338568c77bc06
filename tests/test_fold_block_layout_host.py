"""CPU test of the fold block's appended region (csrc/ggd_binning_layout.h): the instances per tile row, REPS x 64 words BEHIND the
level-1 status words, addressed by ggd_fold_rowinst_offset / ggd_fold_block_words.  tests/host/fold_block_layout.cpp -- a
stand-alone program -- is compiled with the system C++ compiler and -fsanitize=address,undefined and run as a child process: it
writes the level-1 status rows and the new region into a block of exactly ggd_fold_block_words(P) words.  The expected figures are
restated here from the formulas test_binning_layout_host.py pins; nothing is imported from the code under test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gaussian_gan_decoder_amd", "csrc")
PS = [1, 255, 1024, 1025, 4096, 4097, 16 * 1024, 16 * 1024 + 1, 4096 * 256, 4096 * 256 + 1, 4096 * 257, 1_000_000, 5_000_000]
REPS = 16


def gshift(n):
    g = 2
    while (1 << (2 * g)) < n:
        g += 1
    return g


def l1_offset(P):
    tiles = max((P + 4095) // 4096, 1)
    return (16 * 1280 + 64 + REPS * 64) + 4 * (tiles + (1 << gshift(tiles)) + 1) * 256


def l1_end(P):
    chunks = (P + 1023) // 1024
    return l1_offset(P) + (chunks + (1 << gshift(max(chunks, 1))) + 2) * 64


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    cxx = next((c for c in (os.environ.get("CXX"), shutil.which("g++"), shutil.which("c++"), shutil.which("clang++"),
                            "/opt/rocm/llvm/bin/clang++") if c and (shutil.which(c) or os.path.exists(c))), None)
    assert cxx, "no C++ compiler found"
    exe = str(tmp_path_factory.mktemp("foldblock") / "fold_block_layout")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, os.path.join(ROOT, "tests", "host", "fold_block_layout.cpp"), "-o", exe], check=True)
    res = subprocess.run([exe], input="".join(f"{P}\n" for P in PS), capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stderr == "", res.stderr
    out = [{k: int(v) for k, v in (kv.split("=") for kv in line.split())} for line in res.stdout.splitlines()]
    assert [r["P"] for r in out] == PS
    return out


def test_the_region_starts_behind_the_level1_status_words(rows):
    for r in rows:
        assert r["l1_offset"] == l1_offset(r["P"]) and r["l1_end"] == l1_end(r["P"])
        assert r["rowinst_offset"] >= r["l1_end"], r
        assert r["overlap"] == 0 and r["ones"] == r["l1_end"] - r["l1_offset"] and r["twos"] == REPS * 64, r


def test_the_region_fits_inside_the_allocated_block(rows):
    """fold_prepare allocates, clears and marks dirty ggd_fold_block_words(P) words (the program wrote the whole region into a
    heap block of exactly that size under AddressSanitizer)"""
    for r in rows:
        assert r["rowinst_offset"] + REPS * 64 <= r["block_words"], r
        assert r["block_words"] == l1_end(r["P"]) + REPS * 64, r


def test_the_pinned_figures_are_unchanged(rows):
    for r in rows:
        assert r["ctl_words"] == l1_end(r["P"]), r
        assert (r["rowtot"], r["head"], r["reps"]) == (16 * 1280 + 64, 16 * 1280 + 64 + REPS * 64, REPS)
        assert (r["tab_rowstart"], r["tab_rowblk"], r["tab_tilestart"], r["tab_rowinst"], r["tab_flag"], r["tab_words"]) == \
               (0, 65, 130, 130 + 4096, 130 + 4096 + 64, 130 + 4096 + 128)


def test_the_host_bound_admits_the_cube_and_the_shell(rows):
    """launched level-2 blocks of the two 1 M / 1024^2 scenes at their capacities (5 931 642 and 16 777 217 instances)"""
    r = rows[0]
    assert r["blocks_cube"] == 5857 and r["blocks_shell"] == 16449
    assert r["blocks_shell"] <= r["max_blocks"] == (1 << 24) // 1024 + 128
