"""CPU-only: BufRegistry (scroll-prover_amd/csrc/buf_registry.hpp), the bookkeeping behind mi355_buf_alloc / _free / _trim and the order in which an allocation tries the pool,
the slabs' free ranges, a recycle of the pool and a new slab, compiled into the stand-alone tests/hostcheck/buf_registry_main.cpp under -fsanitize=address,undefined and run as
a program of its own: random alloc / free / recycle / trim sequences on two slots through the registry's own allocation decision, against a byte map."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bufreg") / "buf_registry_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "hostcheck", "buf_registry_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    return dict(line.split()[:2] for line in out.stdout.splitlines() if len(line.split()) >= 2)


@pytest.mark.parametrize("prop", [
    "live_pooled_free_never_overlap", "no_two_ranges_start_together", "every_slab_byte_is_live_pooled_or_free", "live_is_what_the_caller_holds", "live_bytes_per_slot",
    "interior_pointer_finds_its_owner", "pointer_into_free_memory_finds_nothing", "range_check_accepts_to_the_end", "range_check_rejects_one_past_the_end",
    "freed_block_is_reused_for_its_size", "small_block_not_in_dedicated_slab", "all_freed_every_slab_is_one_range", "all_freed_every_slab_goes_back",
    "drain_of_one_slot_moves_nothing_of_the_other", "drain_empties_the_slots_pool", "base_pointer_frees", "second_free_is_refused", "pool_key_matches_block",
    "recycle_asked_once", "new_slab_serves_the_request", "slab_size_and_kind", "direct_only_without_slabs", "direct_blocks_are_not_carved", "device_memory_freed_once",
    "take_all_takes_live_and_pooled_of_one_slot"])
def test_registry_property(report, prop):
    assert report[prop] == "ok"
