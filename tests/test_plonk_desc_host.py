"""sipp_amd/csrc/plonk_desc.hpp on its own: the one reading of the outer prover's descriptions that the prover (plonk.hip, lookup.hip,
circuit_data.hip) and the host-only verifier (verify.cpp) both trust, compiled alone into tests/host/plonk_desc_check.cpp with
AddressSanitizer / UBSan and fed the catalogues that pin the refusals on the GPU side: every reason maps to the status the catalogue names.
The mapping tables below are copied from lookup_check (lookup.hip) and check() (plonk.hip) as they stood before the header existed."""
import os
import subprocess

import pytest

from tests import _lookup_cases as lc
from tests import _lookup_tables_cases as tc
from tests import _perm_cases as pc

OK, E_BADARG, E_UNSUPPORTED = 0, lc.E_BADARG, lc.E_UNSUPPORTED
LOOKUP_STATUS = {"ok": OK, "too_many_slots": E_UNSUPPORTED, "empty_with_tag": E_BADARG, "one_sided": E_BADARG, "circuit_sizes": E_BADARG,
                 "column_outside": E_BADARG, "marker_is_selector": E_BADARG, "tag_columns": E_BADARG}
PARAMS_STATUS = {"ok": OK, "bad_argument": E_BADARG, "chunk_size": E_UNSUPPORTED, "counts": E_UNSUPPORTED}
# the reason behind a catalogue row where the status alone does not tell the refusals apart (lookup_check's order)
LOOKUP_REASON = {"q_look_outside": "column_outside", "q_tab_outside": "column_outside", "looking_wires_run_outside": "column_outside",
                 "look_wire0_huge": "column_outside", "table_constants_run_outside": "column_outside",
                 "multiplicity_wires_run_outside": "column_outside", "q_look_is_a_selector": "marker_is_selector",
                 "q_tab_is_a_selector": "marker_is_selector", "looks_without_table": "one_sided", "table_without_looks": "one_sided",
                 "last_word_not_zero": "tag_columns", "n_look_129": "too_many_slots", "n_tab_129": "too_many_slots",
                 "tag_column_is_a_selector": "tag_columns", "second_tag_column_outside": "tag_columns", "tag_columns_outside": "tag_columns",
                 "tag_word_huge": "tag_columns", "empty_description_with_tags": "empty_with_tag"}


@pytest.fixture(scope="module")
def check():
    host = os.path.join(os.path.dirname(__file__), "host")
    subprocess.check_call(["make", "-C", host, "-s", "plonk_desc_check_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")

    def run(lines):
        out = subprocess.run([os.path.join(host, "plonk_desc_check_asan")], input="".join(l + "\n" for l in lines), capture_output=True, text=True,
                             timeout=60, env=env)
        assert out.returncode == 0 and out.stderr == "", out.stdout + out.stderr
        answers = out.stdout.split("\n")[:-1]
        assert len(answers) == len(lines)
        return answers
    return run


def lookup_rows():
    """(name, description, the status the catalogue names; None = served)"""
    rows = [("good", lc.GOOD_DESC, None), ("all_zero", (0,) * 8, None)]
    rows += [(name, desc, None) for name, desc in lc.SERVED_AT_THE_EDGE]
    return rows + list(lc.REFUSALS) + list(tc.TAG_WORDS)


def test_the_catalogues_reach_the_edges_of_the_lookup_validator():
    s, by_name = lc.REFUSAL_SHAPE, {name: (desc, code) for name, desc, code in lookup_rows()}
    assert len(by_name) == len(lookup_rows())
    desc, code = by_name["looking_wires_end_at_the_last_wire"]
    assert desc[1] + 2 * desc[2] == s["num_wires"] and code is None
    desc, code = by_name["looking_wires_run_outside"]
    assert desc[1] + 2 * desc[2] == s["num_wires"] + 1 and code == E_BADARG
    desc, code = by_name["last_two_columns"]
    assert desc[7] + 1 == s["num_constants"] - 1 and code is None
    assert by_name["n_look_129"][0][2] == 129 and by_name["n_tab_129"][0][6] == 129


def test_every_lookup_reason_maps_to_the_catalogues_status(check):
    s, rows = lc.REFUSAL_SHAPE, lookup_rows()
    answers = check(["lookup %d %d %d " % (s["num_wires"], s["num_constants"], s["num_selectors"]) + " ".join(str(w) for w in desc)
                     for _, desc, _ in rows])
    for (name, _, code), reason in zip(rows, answers):
        assert LOOKUP_STATUS[reason] == (OK if code is None else code), (name, reason)
        assert reason == LOOKUP_REASON.get(name, "ok"), (name, reason)
    assert {r for r in answers} >= set(LOOKUP_STATUS) - {"circuit_sizes"}


def test_the_circuit_sizes_reason_is_the_size_caps(check):
    w = " ".join(str(x) for x in lc.GOOD_DESC)
    assert check(["lookup 4096 1024 2 " + w, "lookup 4097 1024 2 " + w, "lookup 4096 1025 2 " + w, "lookup 8 8 9 " + w,
                  "lookup 4097 1024 2 0 0 0 0 0 0 0 0"]) == ["ok", "circuit_sizes", "circuit_sizes", "circuit_sizes", "ok"]


def test_every_parameter_reason_maps_to_the_catalogues_status(check):
    answers = check(["params %d %d %d %d" % (R, D, C, log_n) for _, log_n, R, D, C, _ in pc.REFUSALS_A])
    for (name, _, _, _, _, code), reason in zip(pc.REFUSALS_A, answers):
        assert PARAMS_STATUS[reason] == code, (name, reason)
    assert set(answers) == set(PARAMS_STATUS) - {"ok"}
    # served, with log_d and the chunk count: the shapes of the permutation catalogue
    shapes = [(R, D, C) for R, D, C, _ in pc.SHAPES]
    assert check(["params %d %d %d 5" % s for s in shapes]) == ["ok %d %d" % (D.bit_length() - 1, (R + D - 1) // D) for R, D, C in shapes]
