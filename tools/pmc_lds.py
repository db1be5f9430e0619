#!/usr/bin/env python3
"""Runs ON THE GPU BOX: how busy the LDS pipe is under k_step_implicit_fast, from hardware counters, for one bench config.

  [ADCRAFT_HIP_LIB=<another build>] python3 tools/pmc_lds.py <cfg> <outdir>

A sibling of tools/pmc_issue_stream.py: one rocprofv3 --pmc pass of `python3 bench.py --config <cfg>`, counters only and one env
group.  The LDS counters wanted are asked of `rocprofv3 -L` first, and those the device does not offer are left out (and named in
the record).  Units: SQ_ACTIVE_INST_LDS and SQ_WAIT_INST_LDS are quad-cycles summed over waves, as the other SQ wave
counters (MI355X_MICROARCH.md).  SQ_LDS_IDX_ACTIVE and SQ_LDS_BANK_CONFLICT count the LDS array's busy cycles per CU, summed over CUs;
no document at hand gives their unit, and it is taken to be cycles by inference: on cfg2 the quad-cycle reading puts the array at
233 % of the kernel's cycles, the cycle reading at 58 % - the record carries both.  GRBM_GUI_ACTIVE is the kernel's cycles, summed
over the eight XCDs."""
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
WANTED = ["SQ_INSTS_LDS", "SQ_ACTIVE_INST_LDS", "SQ_WAIT_INST_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_LDS_IDX_ACTIVE", "SQ_INSTS_VALU", "GRBM_GUI_ACTIVE",
          "SQ_BUSY_CU_CYCLES"]
listing = subprocess.run(["rocprofv3", "-L"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120).stdout
counters = [c for c in WANTED if c in listing]
missing = [c for c in WANTED if c not in counters]
d = os.path.join(out, f"{cfg}_lds")
cmd = ["rocprofv3", "--pmc", *counters, "--output-format", "csv", "-d", d, "-o", "pmc", "--", "python3", "bench.py", "--config", cfg,
       "--steps", "12", "--warmup", "2", "--spin-seconds", "0", "--no-cpu-baseline", "--full"]
with open(os.path.join(out, f"{cfg}_lds.log"), "w") as log:
    try:
        rc = subprocess.call(cmd, stdout=log, stderr=subprocess.STDOUT, env=dict(os.environ, ADCRAFT_STREAM_GROUPS="1"), timeout=180)
    except subprocess.TimeoutExpired:          # (subprocess.call has killed the child: nothing more is started on the device)
        sys.exit(124)
if rc != 0:          # (a fault of the profiled run ends the collection: nothing more is started on the device)
    sys.exit(128 - rc if rc < 0 else rc)
acc = collections.defaultdict(list)
for f in glob.glob(d + "/**/*counter_collection.csv", recursive=True):
    for r in csv.DictReader(open(f)):
        if "k_step_implicit" in r["Kernel_Name"]:
            acc[r["Counter_Name"]].append(float(r["Counter_Value"]))
m = {k: sum(v) / len(v) for k, v in acc.items()}
cus = 256          # MI355X
kernel_cycles = m["GRBM_GUI_ACTIVE"] / 8.0
derived = {"kernel_cycles": kernel_cycles, "lds_per_valu": m["SQ_INSTS_LDS"] / m["SQ_INSTS_VALU"],
           "lds_instructions_per_cu": m["SQ_INSTS_LDS"] / cus,
           "kernel_cycles_per_lds_instruction_and_cu": kernel_cycles / (m["SQ_INSTS_LDS"] / cus),
           "quad_cycles_per_lds_instruction": m["SQ_ACTIVE_INST_LDS"] / m["SQ_INSTS_LDS"]}
if "SQ_LDS_IDX_ACTIVE" in m:
    # the LDS array's busy cycles per CU over the kernel's cycles, both readings of the counter's unit (cycles, or quad-cycles as
    # the other SQ cycle counters are): the one that stays below 1 with SQ_LDS_BANK_CONFLICT inside it is the unit
    derived["lds_busy_share_if_cycles"] = m["SQ_LDS_IDX_ACTIVE"] / (cus * kernel_cycles)
    derived["lds_busy_share_if_quad_cycles"] = 4.0 * m["SQ_LDS_IDX_ACTIVE"] / (cus * kernel_cycles)
    derived["lds_array_cycles_per_instruction"] = m["SQ_LDS_IDX_ACTIVE"] / m["SQ_INSTS_LDS"]
    if "SQ_LDS_BANK_CONFLICT" in m:
        derived["bank_conflict_share_of_lds_active"] = m["SQ_LDS_BANK_CONFLICT"] / m["SQ_LDS_IDX_ACTIVE"]
rec = {"config": cfg, "library": os.environ.get("ADCRAFT_HIP_LIB", "product"), "dispatches": len(acc["SQ_INSTS_LDS"]), "not_offered": missing,
       "per_launch": m, "derived": derived}
with open(os.path.join(out, f"lds_{cfg}.json"), "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps(rec, indent=1))
