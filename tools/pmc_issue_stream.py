#!/usr/bin/env python3
"""Runs ON THE GPU BOX: what a wave of k_step_implicit_fast spends its issue turns on, from hardware counters, for one bench config.

  [ADCRAFT_HIP_LIB=<another build>] python3 tools/pmc_issue_stream.py <cfg> <outdir>

Two rocprofv3 --pmc passes of `python3 bench.py --config <cfg>` (eight SQ counters fit one pass), counters only and one env group, as
tools/pmc_collect.py takes its own: instruction counts by kind and the cycles the waves spend on each (pass `insts`), then the wait
and issue-stall buckets MI355X_MICROARCH.md lists under SQ (pass `waits`: WAIT_ANY + WAIT_INST_ANY + ACTIVE_INST_ANY make up
WAVE_CYCLES).  SQ_* cycle counters are in quad-cycles and summed over waves; GRBM_GUI_ACTIVE is the kernel's cycles."""
import collections
import csv
import glob
import json
import os
import subprocess
import sys

cfg, out = sys.argv[1], sys.argv[2]
os.makedirs(out, exist_ok=True)
os.environ["TMPDIR"] = "/tmp"
PASSES = {"insts": ["SQ_WAVES", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_VALU", "SQ_WAVE_CYCLES", "SQ_INSTS_SALU", "SQ_INSTS_LDS", "SQ_ACTIVE_INST_LDS", "GRBM_GUI_ACTIVE"],
          "waits": ["SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "SQ_WAIT_INST_LDS", "SQ_ACTIVE_INST_ANY", "SQ_ACTIVE_INST_SCA", "SQ_ACTIVE_INST_MISC", "SQ_INSTS_BRANCH", "SQ_BUSY_CU_CYCLES"]}
acc = collections.defaultdict(list)
for name, counters in PASSES.items():
    d = os.path.join(out, f"{cfg}_{name}")
    cmd = ["rocprofv3", "--pmc", *counters, "--output-format", "csv", "-d", d, "-o", "pmc", "--", "python3", "bench.py", "--config", cfg,
           "--steps", "12", "--warmup", "2", "--spin-seconds", "0", "--no-cpu-baseline", "--full"]
    with open(os.path.join(out, f"{cfg}_{name}.log"), "w") as log:
        rc = subprocess.call(cmd, stdout=log, stderr=subprocess.STDOUT, env=dict(os.environ, ADCRAFT_STREAM_GROUPS="1"))
    if rc != 0:          # (a fault of the profiled run ends the collection: nothing more is started on the device)
        sys.exit(128 - rc if rc < 0 else rc)
    for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
        for r in csv.DictReader(open(f)):
            if "k_step_implicit" in r["Kernel_Name"]:
                acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
m = {k: sum(v) / len(v) for k, v in acc.items()}
simds = 4 * 256          # MI355X: 256 CUs of four SIMDs
kernel_cycles = m["GRBM_GUI_ACTIVE"] / 8.0          # (the counter is summed over the eight XCDs: 3.55e6 for a 0.185-ms launch at 2.4 GHz)
rec = {"config": cfg, "library": os.environ.get("ADCRAFT_HIP_LIB", "product"), "dispatches": len(acc["SQ_WAVES"]), "per_launch": m,
       "derived": {
           "kernel_cycles": kernel_cycles,
           "valu_busy_share_of_kernel_cycles": 4.0 * m["SQ_ACTIVE_INST_VALU"] / (simds * kernel_cycles),
           "mean_waves_per_simd": 4.0 * m["SQ_WAVE_CYCLES"] / (simds * kernel_cycles),
           "valu_share_of_wave_cycles": m["SQ_ACTIVE_INST_VALU"] / m["SQ_WAVE_CYCLES"],
           "quad_cycles_per_valu_instruction": m["SQ_ACTIVE_INST_VALU"] / m["SQ_INSTS_VALU"],
           "kernel_cycles_per_valu_instruction_and_simd": kernel_cycles / (m["SQ_INSTS_VALU"] / simds),
           "salu_per_valu": m["SQ_INSTS_SALU"] / m["SQ_INSTS_VALU"], "lds_per_valu": m["SQ_INSTS_LDS"] / m["SQ_INSTS_VALU"],
           "branch_per_valu": m["SQ_INSTS_BRANCH"] / m["SQ_INSTS_VALU"],
           "wait_any_share": m["SQ_WAIT_ANY"] / m["SQ_WAVE_CYCLES"], "wait_inst_any_share": m["SQ_WAIT_INST_ANY"] / m["SQ_WAVE_CYCLES"],
           "wait_inst_lds_share": m["SQ_WAIT_INST_LDS"] / m["SQ_WAVE_CYCLES"], "active_inst_any_share": m["SQ_ACTIVE_INST_ANY"] / m["SQ_WAVE_CYCLES"],
           "active_inst_scalar_share": m["SQ_ACTIVE_INST_SCA"] / m["SQ_WAVE_CYCLES"], "active_inst_branch_share": m["SQ_ACTIVE_INST_MISC"] / m["SQ_WAVE_CYCLES"]}}
with open(os.path.join(out, f"issue_stream_{cfg}.json"), "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps(rec, indent=1))
