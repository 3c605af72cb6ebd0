"""CPU-only: WsLayout (scroll-prover_amd/csrc/ws_layout.hpp), the bump allocator that places the fields of the pooled workspace blocks of lib_aux.hip and lib_pairing.hip,
compiled into the stand-alone tests/hostcheck/ws_layout_main.cpp under -fsanitize=address,undefined and run as a program of its own.  Random sequences of field sizes
(every take() offset a multiple of 256, fields disjoint and in order, last end <= total() < last end + 256), the sizes 0, 1, 255, 256, 257 and 2^40, and for the six
entry points laid out with it the block size against the hand-added offset chain each of them had before."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wslayout") / "ws_layout_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "hostcheck", "ws_layout_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    verdicts = {}
    for line in out.stdout.splitlines():
        w = line.split()
        if len(w) >= 2 and w[1] in ("ok", "WRONG"):
            verdicts.setdefault(w[0], []).append(w[1])
    return verdicts


def test_random_sequences_are_aligned_disjoint_and_bounded(report):
    for name in ("random_take_offsets_aligned", "random_take_fields_disjoint", "random_take_total_bounds", "random_mixed_in_order"):
        assert report[name] == ["ok"], name


def test_edge_sizes_and_64_bit_offsets(report):
    for name in ("size_0_takes_no_room", "size_1", "size_255", "size_256", "size_257", "size_2_pow_40", "total_past_2_pow_40", "take_exact_is_exact"):
        assert report[name] == ["ok"], name


@pytest.mark.parametrize("entry", ["lookup", "sigma", "nonzero_rows", "copy_check", "pairing", "poseidon"])
def test_block_size_equals_the_hand_added_chain(report, entry):
    assert report[entry + "_bytes_unchanged"] == ["ok"]
