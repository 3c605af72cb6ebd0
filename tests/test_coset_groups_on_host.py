"""CPU-only: plonk::detail::coset_groups (include/mi355zk_plonk.hpp), the greedy cut of a compiled quotient plan into consecutive groups of launches whose coset parts
ProofOptions::coset_group_polys transforms one group at a time.  tests/hostcheck/coset_groups_main.cpp, built under -fsanitize=address,undefined, compiles the plans of all seven
layers (scroll-prover_amd/protocols.py) and of the reference's two fixtures and cuts each with G in {24, 25, 40, 64, all}, key resident and lean.  Also the surface of the memory
limit: the three new symbols in the header, the ctypes table and the Rust binding, and the defaults of the new options."""
import os
import re
import subprocess

import pytest

import __graft_entry__ as ge

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NEW_SYMBOLS = ("mi355_mem_set_limit", "mi355_mem_usage", "mi355_mem_reset_peak")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cosetgroups")
    zk = ge.load_package()
    files = []
    for layer in range(7):
        files.append(str(tmp / f"layer{layer}.json"))
        zk.protocols.write(layer, files[-1])
    files += [os.path.join(HERE, "golden", "protocol_layer2.json"), os.path.join(HERE, "golden", "protocol_layer4.json")]
    exe = str(tmp / "coset_groups_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(HERE, "hostcheck", "coset_groups_main.cpp")])
    out = subprocess.run([exe] + files, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    return dict(line.split()[:2] for line in out.stdout.splitlines() if len(line.split()) >= 2 and not line.startswith("#"))


@pytest.mark.parametrize("prop", [
    "groups_are_consecutive_in_order_and_cover_every_launch_once", "every_launch_operand_lies_in_its_group", "no_group_exceeds_G", "all_gives_one_group_and_no_retransform",
    "more_than_G_operands_give_two_groups_or_more", "G_23_is_refused", "retransforms_are_the_repeated_members", "groups_are_greedy", "resident_key_counts_witness_only",
    "seven_layers_and_two_fixtures"])
def test_grouping_property(report, prop):
    assert report[prop] == "ok"


def test_new_symbols_are_in_the_header_the_ctypes_table_and_the_rust_binding():
    header = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    rust = open(os.path.join(ROOT, "rust_shim", "mi355zk.rs")).read()
    zk = ge.load_package()
    for s in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % s, header), s
        assert s in zk._capi.SIGNATURES, s
        assert re.search(r"pub fn %s\s*\(" % s, rust), s
    for f in ("mem_set_limit", "mem_usage", "mem_reset_peak"):
        assert callable(getattr(zk.halo2, f))
    cpp = open(os.path.join(ROOT, "include", "mi355zk_halo2.hpp")).read()
    assert "mem_set_limit" in cpp and "mem_usage" in cpp


def test_no_new_environment_variable():
    """the limit is set by a call: nothing under csrc/ or include/ reads a variable named after it"""
    for d in ("scroll-prover_amd/csrc", "include"):
        for name in os.listdir(os.path.join(ROOT, d)):
            txt = open(os.path.join(ROOT, d, name), errors="replace").read()
            assert not re.search(r'getenv\("MI355_(MEM|HBM|COSET_GROUP)', txt), name


def test_proof_options_default_is_the_ungrouped_path(tmp_path):
    src = tmp_path / "defaults.cpp"
    src.write_text('#include "mi355zk_plonk.hpp"\n#include <cstdio>\nint main() { mi355zk::plonk::ProofOptions o; mi355zk::plonk::ProofResult r;\n'
                   '  std::printf("%u %u %u\\n", o.coset_group_polys, r.coset_groups, r.coset_retransforms); return 0; }\n')
    exe = str(tmp_path / "defaults")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-pthread", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    assert subprocess.run([exe], capture_output=True, text=True, timeout=60).stdout.split() == ["0", "0", "0"]
