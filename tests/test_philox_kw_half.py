"""adc_law.h philox4x32_kw / draw_kw (the dense fast pass's stage-B conversion draw, started from the keyword's half of round 1
that phase 1 keeps per keyword) give the bits of philox4x32 / draw: checked on the host build of the header (plain C++)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = shutil.which("c++") or shutil.which("g++")

PROGRAM = r"""
#include <stdio.h>
#include "adc_law.h"
int main()
{
    uint64_t s = 0x9E3779B97F4A7C15ull;
    auto next = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return s; };
    long bad = 0;
    for (int i = 0; i < 200000; ++i) {
        const uint64_t key = next();
        const uint64_t r = next();
        const uint32_t index = (uint32_t)r & 0x00FFFFFFu, keyword = (uint32_t)(r >> 32), tick = (uint32_t)next();
        const uint32_t stage = i % 3 == 0 ? (uint32_t)adc::ST_CONV : (uint32_t)(r >> 24) & 15u;
        const adc::U4 a = adc::draw(key, index, stage, keyword, tick);
        const adc::U4 b = adc::draw_kw(key, index, adc::philox_kw_half(stage, keyword, (uint32_t)key), tick);
        bad += a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w;
    }
    for (uint32_t a = 0; a < 4096; ++a) {                               // xor_and: a ^ (b & c)
        const uint32_t x = (uint32_t)next(), y = (uint32_t)next(), z = (uint32_t)next();
        bad += adc::xor_and(x, y, z) != (x ^ (y & z));
    }
    printf("%ld\n", bad);
    return 0;
}
"""


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
def test_draw_from_the_keyword_half_equals_draw(tmp_path):
    src, exe = tmp_path / "kw_half.cpp", tmp_path / "kw_half"
    src.write_text(PROGRAM)
    subprocess.check_call([CXX, "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "adcraft_amd", "csrc"), str(src), "-o", str(exe)])
    assert subprocess.check_output([str(exe)], text=True).strip() == "0"
