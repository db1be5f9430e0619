#!/usr/bin/env python
"""Record what every exported adc_*_config_check, adc_*_pop_config_check and adc_replay_nstep_check answers to the cases of
tests/config_message_cases.py - (function, case, return code, message) - into tests/golden/config_check_messages.json.

The refusal sentences are part of what callers see (engine.py raises them as they are), and most are matched by no test or by a
fragment only.  Run this BEFORE a change that touches how the checks are written, commit the JSON unchanged, and
tests/test_config_messages_host.py holds the change to the same codes and the same whole sentences, against the library and the
g++ host build alike.  No GPU is needed: the checks are host code.

    python tools/gen_golden_config_messages.py            # writes tests/golden/config_check_messages.json
    python tools/gen_golden_config_messages.py --check    # compares instead of writing; exit status 1 on a difference
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from adcraft_amd import _ffi  # noqa: E402
from tests import config_message_cases as cases  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "config_check_messages.json")


def main():
    rows = cases.run(_ffi.lib())
    names = [(r[0], r[1]) for r in rows]
    assert len(set(names)) == len(names), "case names must be unique within a function"
    if "--check" in sys.argv:
        want = cases.load(OUT)
        bad = [(w, r) for w, r in zip(want, rows) if w != r]
        for w, r in bad:
            print("recorded", w, "\n     now", r)
        print(f"{len(rows)} cases, {len(want)} recorded, {len(bad)} differ")
        sys.exit(1 if bad or len(want) != len(rows) else 0)
    cases.dump(rows, OUT)
    print(f"{len(rows)} cases, {len({r[3] for r in rows if r[3]})} distinct messages -> {os.path.relpath(OUT, ROOT)}")


if __name__ == "__main__":
    main()
