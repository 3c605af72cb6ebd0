"""CPU-only: the table of the library's init-time environment variables (scroll-prover_amd/csrc/knobs.hpp).
  * tests/hostcheck/knobs_main.cpp, a stand-alone program under -fsanitize=address,undefined: for every variable and every input string the table yields field for field what the
    getenv lines it replaced yield (those lines are carried there verbatim), moves no other field, and starts from the same defaults;
  * the names: DESIGN.md section 10 lists exactly the variables the code reads -- the rows of knobs.hpp plus every "MI355_..." literal under csrc/ -- in both directions."""
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "scroll-prover_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("knobs") / "knobs_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-o", exe, os.path.join(HERE, "hostcheck", "knobs_main.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr
    return dict(line.split()[:2] for line in out.stdout.splitlines() if len(line.split()) >= 2 and not line.startswith("#"))


def table_names():
    with open(os.path.join(CSRC, "knobs.hpp")) as f:
        return re.findall(r'^\s*X\(\w+, \w+, "(MI355_[A-Z0-9_]+)"', f.read(), re.M)


def test_table_has_the_33_variables_once_each(report):
    names = table_names()
    assert len(names) == 33 and len(set(names)) == 33
    assert report["table_has_33_rows"] == "ok" and report["names_are_distinct"] == "ok"


def test_defaults_are_the_earlier_member_initialisers(report):
    assert report["defaults_equal_the_earlier_initialisers"] == "ok"


def test_every_variable_parses_as_before_and_moves_no_other_field(report):
    wrong = [n for n in table_names() if report.get(n) != "ok"]
    assert not wrong and report["all_set_together"] == "ok", wrong


def test_design_section_10_lists_exactly_the_variables_the_code_reads():
    code = set(table_names())
    for name in sorted(os.listdir(CSRC)):
        with open(os.path.join(CSRC, name), errors="replace") as f:
            text = f.read()
        assert not re.search(r"getenv\(\s*[a-z_]+\s*\)", text) or name in ("lib_aux.hip", "lib_core.hip"), name    # a getenv of a computed name would escape the literals below
        code |= set(re.findall(r'"(MI355_[A-Z0-9_]+)"', text))
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    section = design[design.index("\n## 10. "):design.index("\n## 11. ")]
    rows = [line for line in section.splitlines() if line.startswith("| `MI355_")]
    documented = [re.match(r"\| `(MI355_[A-Z0-9_]+)` \|", line).group(1) for line in rows]
    assert len(documented) == len(set(documented))
    assert set(documented) - code == set(), "documented, but no code reads it"
    assert code - set(documented) == set(), "read by the code, but not in DESIGN.md section 10"
    assert len(code) == 33 + 4
