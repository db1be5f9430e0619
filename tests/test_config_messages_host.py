"""The refusal sentences of every exported adc_*_config_check, adc_*_pop_config_check and adc_replay_nstep_check, whole: the cases
of tests/config_message_cases.py replayed against tests/golden/config_check_messages.json (tools/gen_golden_config_messages.py
recorded it before the checks' shared clauses were given one body) - the return code and the sentence of the first failing clause
are equal for every case, in the library hipcc builds and in the g++ host build of the same source."""
import ctypes as C
import os

import pytest

from tests import config_message_cases as cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "config_check_messages.json")


def _library():
    from adcraft_amd import _ffi
    return _ffi.lib()


def _host_build():
    from oracle import build as obuild
    return C.CDLL(obuild.build_shims_host())


@pytest.fixture(scope="module")
def recorded():
    return cases.load(GOLDEN)


@pytest.mark.parametrize("load", [_library, _host_build], ids=["library", "host-build"])
def test_every_case_answers_the_recorded_code_and_sentence(load, recorded):
    rows = cases.run(load())
    assert [r[:2] for r in rows] == [r[:2] for r in recorded], "the case list and the recorded file differ: tools/gen_golden_config_messages.py"
    wrong = [(want, got) for want, got in zip(recorded, rows) if want != got]
    assert not wrong, f"{len(wrong)} of {len(rows)} cases differ; the first: recorded {wrong[0][0]}, now {wrong[0][1]}"


def test_the_record_covers_every_function_and_both_outcomes(recorded):
    by_fn = {}
    for fn, _, rc, msg in recorded:
        assert (rc == 0) == (msg is None), (fn, rc, msg)
        by_fn.setdefault(fn, set()).add(rc)
    assert set(by_fn) == set(cases.SIGNATURES)
    assert all(codes == {0, -1} for codes in by_fn.values()), by_fn
