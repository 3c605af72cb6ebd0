"""CPU-only: csrc/plonk_capi.hpp -- the handle table, the option parser and the JSON record writer behind the mi355_plonk_* entry points -- compiled into the stand-alone
tests/hostcheck/plonk_capi_main.cpp under -fsanitize=address,undefined and run as a program of its own: random issue / free / lookup sequences against a model, stale and
wrong-kind handles, every option name with good and bad values (bad hexadecimal included), and the writer on extreme values, whose output this test holds to json.loads."""
import json
import math
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("plonk_capi") / "plonk_capi_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "hostcheck", "plonk_capi_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    lines = out.stdout.splitlines()
    props = dict(l.split()[:2] for l in lines if not l.startswith("json ") and len(l.split()) >= 2)
    docs = {l.split(" ", 2)[1]: l.split(" ", 2)[2] for l in lines if l.startswith("json ")}
    return props, docs


@pytest.mark.parametrize("prop", [
    "handles_are_issued_in_increasing_order", "a_handle_value_is_never_issued_twice", "lookup_returns_the_issued_object", "wrong_kind_is_refused_and_names_the_expected_kind",
    "kind_of_a_live_handle", "a_held_object_outlives_its_handle", "a_freed_handle_is_refused", "a_second_free_is_refused", "kind_of_a_freed_handle_is_none", "a_stale_handle_stays_refused",
    "live_count_follows_the_model", "a_never_issued_handle_is_refused", "handle_zero_is_refused", "issued_counts_every_handle", "everything_freed_nothing_alive", "nothing_to_issue_is_refused",
    "bool_options_parse", "bad_bool_is_refused_by_name", "int_options_parse", "out_of_range_int_is_refused_by_name", "bad_int_is_refused_by_name", "uint_options_parse",
    "out_of_range_uint_is_refused_by_name", "bad_uint_is_refused_by_name", "hex_options_parse_in_byte_order", "hex_options_accept_upper_case", "bad_hex_is_refused_by_name",
    "transcript_names_parse", "bad_transcript_is_refused_by_name", "a_refused_value_leaves_the_option_as_it_was", "unknown_option_is_named", "unprintable_names_are_masked",
    "null_name_or_value_is_refused", "unset_options_are_absent", "cap_zero_asks_for_the_size", "copy_out_copies", "a_small_buffer_is_refused_and_untouched", "null_outputs_are_refused",
    "writer_is_complete_after_the_last_close", "writer_refuses_a_value_without_a_key", "writer_refuses_a_key_in_an_array", "writer_refuses_a_mismatched_close",
    "writer_refuses_two_top_level_values", "writer_refuses_to_print_an_unclosed_document"])
def test_property(run, prop):
    assert run[0][prop] == "ok"


def strict(text):
    def no_constants(name):
        raise AssertionError("not strict JSON: " + name)
    assert text.isascii()
    return json.loads(text, parse_constant=no_constants)


def test_the_writer_is_strict_json_on_extreme_values(run):
    d = strict(run[1]["extremes"])
    assert d["u64_max"] == 2**64 - 1 and d["i64_min"] == -2**63 and d["zero"] == 0
    assert d["nan"] is None and d["inf"] is None and d["ninf"] is None                  # JSON has no NaN and no Infinity
    assert d["dbl_max"] == 1.7976931348623157e308 and d["dbl_min"] == 5e-324 and d["three"] == 3.0 and isinstance(d["three"], float) and d["tenth"] == 0.1
    assert d["neg_zero"] == 0.0 and math.copysign(1, d["neg_zero"]) == -1
    assert d["every_byte"] == "".join(chr(c) for c in range(1, 256))                    # bytes outside printable ASCII travel as \\u00XX, one code point per byte
    assert d['quote"back\\slash\nnewline'] == '"\\\n\t\r\b\f' and d["empty"] == "" and d["nul_inside"] == "a\0b"
    assert d["t"] is True and d["f"] is False and d["null"] is None and d["hex"] == "00ff10"
    assert d["nested"] == [[], {}, [1, -2, {"k": []}]]
    deep = strict(run[1]["deep"])
    for _ in range(200):
        assert isinstance(deep, list) and len(deep) == 1
        deep = deep[0]
    assert deep == 7 and strict(run[1]["scalar"]) == "alone"
