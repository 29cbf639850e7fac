"""Compile warpdemux_amd/csrc/wdx_clip.hip for gfx950 with the Makefile's flags plus -Rpass-analysis=kernel-resource-usage
(nothing runs: no GPU needed) and print one line per clip kernel instantiation: VGPRs, VGPR spills, SGPR spills, scratch
bytes per lane, waves per SIMD, static LDS.  Usage: clip_resource_usage.py [> profiles/clip_resource_usage.txt]"""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "warpdemux_amd", "csrc")


def make_var(text, name):
    m = re.search(r"^%s\s*[:?]?=\s*((?:.*\\\n)*.*)$" % name, text, re.M)
    return m.group(1).replace("\\\n", " ").split() if m else []


def main():
    mk = open(os.path.join(CSRC, "Makefile")).read()
    hipcc = os.environ.get("HIPCC") or make_var(mk, "HIPCC")[0]
    arch = make_var(mk, "ARCH")[0]
    flags = [f.replace("$(ARCH)", arch) for f in make_var(mk, "CXXFLAGS")]
    m = re.search(r"^wdx_clip\.o: CXXFLAGS \+= (.*)$", mk, re.M)  # the unit's own flags
    flags += m.group(1).split() if m else []
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [hipcc] + flags + ["-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(CSRC, "wdx_clip.hip"),
                                 "-o", os.path.join(tmp, "wdx_clip.o")]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True)
    if p.returncode != 0:
        sys.stderr.write(p.stdout)
        return p.returncode
    demangle = lambda s: subprocess.run(["c++filt", s], stdout=subprocess.PIPE, universal_newlines=True).stdout.strip() or s
    print("# %s" % " ".join(os.path.basename(c) if os.sep in c else c for c in cmd[:-3]))
    seen = set()
    for b in re.split(r"remark: [^\n]*Function Name: ", p.stdout)[1:]:
        name = b.split("\n")[0].split(" [-Rpass")[0].strip()
        if name in seen:
            continue
        seen.add(name)

        def g(k):
            m = re.search(k + r": (\S+)", b)
            return m.group(1) if m else "?"

        short = re.sub(r"^void wdx::|\(wdx::ClipArgs\)$|\(.*\)$", "", demangle(name))
        print("%-34s vgpr %3s vgpr_spill %3s sgpr %3s sgpr_spill %3s scratch %4s occ %s lds %s" % (
            short, g("VGPRs"), g("VGPRs Spill"), g("SGPRs"), g("SGPRs Spill"), g(r"ScratchSize \[bytes/lane\]"),
            g(r"Occupancy \[waves/SIMD\]"), g(r"LDS Size \[bytes/block\]")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
