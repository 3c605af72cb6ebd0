"""CPU-only: perm_check (scroll-prover_amd/csrc/perm.hpp), the validation mi355_fr_permutation_sigma_dev runs on the host before anything is uploaded or launched,
compiled into the stand-alone tests/hostcheck/perm_check_main.cpp under -fsanitize=address,undefined and run as a program of its own.  Accepted: the empty list, a
dense list, a 2-cycle, a 17-cycle.  Rejected with the right first index: a cell equal to n_cols * n, an image of 2^64 - 1, a cell listed twice, images that are not
the cells.  flags bit 0 accepts the last two and still rejects the first two."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("permcheck") / "perm_check_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "hostcheck", "perm_check_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    by_flags, cur = {}, None
    for line in out.stdout.splitlines():
        w = line.split()
        if w[0] == "flags":
            cur = by_flags.setdefault(int(w[1]), {})
        elif cur is not None and len(w) >= 3 and w[1] in ("accepted", "rejected"):
            cur[w[0]] = (w[1], int(w[2]))
    return by_flags


@pytest.mark.parametrize("flags", [0, 1])
def test_accepted_lists(report, flags):
    for name in ("empty", "dense", "two_cycle", "seventeen_cycle", "last_cell"):
        assert report[flags][name] == ("accepted", -1), name


@pytest.mark.parametrize("flags", [0, 1])
def test_range_check_always_runs_and_names_the_first_index(report, flags):
    assert report[flags]["cell_equal_to_total"] == ("rejected", 1)
    assert report[flags]["image_all_ones"] == ("rejected", 2)


def test_duplicates_and_bijection_are_rejected_with_the_first_index(report):
    assert report[0]["cell_twice"] == ("rejected", 2)
    assert report[0]["images_not_the_cells"] == ("rejected", 2)
    assert report[0]["image_twice"] == ("rejected", 1)


def test_flag_bit_0_waives_duplicates_and_bijection(report):
    for name in ("cell_twice", "images_not_the_cells", "image_twice"):
        assert report[1][name] == ("accepted", -1), name
