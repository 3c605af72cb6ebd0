"""CPU-only: the yardstick of the device's witness check (tests/witness_check_common.py, MockProver::verify in Python over oracle.plonk) held to planted facts, on
--builder-only dumps of tests/cpp/test_witness_check.cpp at the smallest k tests/test_plonk_protocol.py uses for layers 2 and 4.

  * the builder's instance has no failure of any kind;
  * advice cell (0, 3) -- the output cell of the first vertical gate -- off by one: gate failures only at rows 0 .. 3 of the FIRST gate constraint (the four-row
    neighbourhood that reads the cell), and every copy / lookup failure involves that cell;
  * instance value 0 off by one: the copy constraint that feeds it into a gate input fails, no gate does.
Also: the copy mapping recovered from the sigma columns is a permutation made of the builder's copy pairs."""
import pytest

from tests import witness_check_common as wc

CASES = [(2, 6), (4, 7)]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    root = tmp_path_factory.mktemp("witness_check_reference")
    out = {}
    for layer, k in CASES:
        for name, corrupt in (("clean", ()), ("advice", ("advice:0:3",)), ("instance", ("instance:0",))):
            out[layer, name] = wc.Reference(wc.build_instance(str(root / f"l{layer}_{name}"), layer, k, corrupt))
    return out


@pytest.mark.parametrize("layer,k", CASES)
def test_the_builder_s_instance_has_no_failures(dumps, layer, k):
    ref = dumps[layer, "clean"]
    assert ref.pr.k == k and wc.gate_indices(ref.pr), "the protocol has gates"
    assert ref.gates() == {} and ref.copies() == [] and ref.lookups() == {}
    cells, images = ref.overrides()
    assert len(cells) == 2 * ref.man["copy_pairs"] > 0 and sorted(cells) == sorted(images) and cells == sorted(cells)


@pytest.mark.parametrize("layer,k", CASES)
def test_one_advice_cell_off_breaks_the_first_gate_in_its_four_rows(dumps, layer, k):
    ref = dumps[layer, "advice"]
    gates = ref.gates()
    first = wc.gate_indices(ref.pr)[0]
    assert set(gates) == {first} and gates[first] and set(gates[first]) <= {0, 1, 2, 3}
    assert 0 in gates[first], "row 0's gate reads the cell as its output"
    pos = [j for j, (c, _, _) in enumerate(wc.perm_columns(ref.pr)) if c == ref.pr.phase0[0]]
    for t, ja, ra, jb, rb in ref.copies():
        assert (ja in pos and ra == 3) or (jb in pos and rb == 3)
    assert all(row == 3 for row in ref.lookups().values())


@pytest.mark.parametrize("layer,k", CASES)
def test_one_instance_value_off_breaks_a_copy_and_no_gate(dumps, layer, k):
    ref = dumps[layer, "instance"]
    assert ref.gates() == {} and ref.lookups() == {}
    cp = ref.copies()
    inst_pos = [j for j, (c, _, _) in enumerate(wc.perm_columns(ref.pr)) if c == ref.pr.inst0]
    assert len(inst_pos) == 1 and len(cp) == 2, "the 2-cycle through instance cell 0, seen from both of its cells"
    assert all((ja == inst_pos[0] and ra == 0) or (jb == inst_pos[0] and rb == 0) for _, ja, ra, jb, rb in cp)
    clean = dumps[layer, "clean"]
    assert ref.overrides() == clean.overrides(), "the mapping does not depend on the witness"
