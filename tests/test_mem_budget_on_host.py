"""CPU-only: MemLedger (scroll-prover_amd/csrc/mem_budget.hpp), the ledger of the device memory the library holds and the limit mi355_mem_set_limit puts on it, compiled into
the stand-alone tests/hostcheck/mem_budget_main.cpp under -fsanitize=address,undefined and run as a program of its own: random charge / release / reclaim sequences on two slots
through the ledger's own decision, against a plain model."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("membudget") / "mem_budget_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "hostcheck", "mem_budget_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    return dict(line.split()[:2] for line in out.stdout.splitlines() if len(line.split()) >= 2)


@pytest.mark.parametrize("prop", [
    "held_equals_sum_of_classes", "held_is_what_the_driver_holds", "held_never_exceeds_a_limit_it_was_under", "high_water_is_monotone_until_reset", "high_water_is_the_peak_since_reset",
    "reclaim_order_pool_then_tables_then_refuse", "a_refusal_changes_nothing", "slots_are_independent", "limit_zero_refuses_nothing", "lowered_limit_refuses_but_frees_only_by_reclaim",
    "set_limit_frees_nothing", "decision_matches_the_plain_model", "spare_requests_reclaim_nothing", "refusal_names_limit_held_and_request", "release_finds_what_was_bound",
    "second_release_is_refused", "counters_match", "room_is_min_of_free_and_limit_minus_held", "all_released_nothing_held"])
def test_ledger_property(report, prop):
    assert report[prop] == "ok"
