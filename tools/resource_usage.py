#!/usr/bin/env python3
"""Per-kernel register / spill / occupancy table of a HIP source (hipcc -Rpass-analysis=kernel-resource-usage),
compiled with the flags monotonic-rnnt_amd/Makefile gives that file's object (JOINT_FLAGS for the mrnnt_joint* units
included): the table of the kernels the library ships.

usage: python tools/resource_usage.py [--dev] monotonic-rnnt_amd/csrc/mrnnt_grad.hip [filter]
  --dev   the development flavour (-DMRNNT_DEVTOOLS: libmonotonic_rnnt_amd_dev.so)
"""
import re, subprocess, sys, os

here = os.path.dirname(os.path.abspath(__file__))
pkg = os.path.abspath(os.path.join(here, "..", "monotonic-rnnt_amd"))
args = [a for a in sys.argv[1:] if a != "--dev"]
dev = "--dev" in sys.argv[1:]
src = args[0]
flt = args[1] if len(args) > 1 else ""
# the compile line `make` would run for this file's object, with the object and its output left out
obj = os.path.join(pkg, "build", "dev" if dev else "", os.path.splitext(os.path.basename(src))[0] + ".o")
plan = subprocess.run(["make", "-n", "-B", "-C", pkg, obj], capture_output=True, text=True, check=True).stdout
line = next(l for l in plan.splitlines() if " -c " in l and l.rstrip().endswith("-o " + obj))
cmd = line.split()
cmd = cmd[:cmd.index("-c")] + ["-c", os.path.abspath(src), "-o", "/dev/null", "-Rpass-analysis=kernel-resource-usage"]
out = subprocess.run(cmd, capture_output=True, text=True).stderr
rows, cur = [], None
for line in out.splitlines():
    m = re.search(r"remark: +(Function Name|VGPRs|AGPRs|TotalSGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|SGPRs Spill|VGPRs Spill|LDS Size \[bytes/block\]): (\S+)", line)
    if not m:
        continue
    k, v = m.group(1), m.group(2)
    if k == "Function Name":
        dem = subprocess.run(["c++filt", v], capture_output=True, text=True).stdout.strip()
        cur = {"name": dem}
        rows.append(cur)
    elif cur is not None:
        cur[k] = v
for r in rows:
    if flt in r["name"]:
        print(f'{r.get("VGPRs","?"):>4} vgpr {r.get("AGPRs","?"):>3} agpr {r.get("TotalSGPRs","?"):>3} sgpr occ {r.get("Occupancy [waves/SIMD]","?"):>2} '
              f'sspill {r.get("SGPRs Spill","?"):>3} vspill {r.get("VGPRs Spill","?"):>3} scratch {r.get("ScratchSize [bytes/lane]","?"):>4} '
          f'lds {r.get("LDS Size [bytes/block]","?"):>6}  {r["name"]}')
