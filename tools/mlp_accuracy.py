"""Rerun the DTW_MLP tail's GPU accuracy cases (tests/test_gpu_mlp.py) and keep their figures.

    python tools/mlp_accuracy.py profiles/NAME_mlp_accuracy.json
    python tools/mlp_accuracy.py profiles/NAME_boost_accuracy.json tests/test_gpu_boost.py     (the Fpt_Boost tail)

Every case of the test file prints E_ref = max |p_sklearn - p_exact|, T = 4 max(E_ref, u_w), the device's max
|p - p_exact| and its close-call count before it asserts (tests/helpers/mlp_ref.py); this collects those
lines per case, with the largest ratio of device error to E_ref, into one JSON document.
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"(?P<case>[^.:][^:]*): E_ref (?P<e_ref>\S+) T (?P<T>\S+) gpu err (?P<err>\S+) \(x(?P<ratio>\S+) E_ref\) "
                  r"close (?P<close>\d+)/(?P<n>\d+)")


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else None
    tests = sys.argv[2] if len(sys.argv) > 2 else "tests/test_gpu_mlp.py"
    p = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-p", "no:cacheprovider", tests],
                       cwd=ROOT, capture_output=True, text=True)
    cases = []
    for line in p.stdout.splitlines():
        m = LINE.search(line.lstrip("."))
        if m:
            d = m.groupdict()
            cases.append(dict(case=d["case"], e_ref=float(d["e_ref"]), T=float(d["T"]), gpu_max_err=float(d["err"]),
                              err_over_e_ref=float(d["ratio"]), close_calls=int(d["close"]), reads=int(d["n"])))
    ratios = [c["err_over_e_ref"] for c in cases if c["err_over_e_ref"] == c["err_over_e_ref"]]
    res = dict(tool="tools/mlp_accuracy.py", tests=tests, pytest_rc=p.returncode, pytest_tail=p.stdout.strip().splitlines()[-1:],
               cases=cases, max_err_over_e_ref=max(ratios) if ratios else None,
               max_err_over_T=max(c["gpu_max_err"] / c["T"] for c in cases) if cases else None)
    txt = json.dumps(res, indent=1)
    print(txt)
    if out:
        with open(out, "w") as f:
            f.write(txt + "\n")
    sys.exit(p.returncode)


if __name__ == "__main__":
    main()
