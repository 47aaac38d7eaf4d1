#!/usr/bin/env python3
"""Print the argument-rule sweep of tests/test_entry_rules_host.py (every entry family but the merge, which has its own sweep): the status
each build returned for every case. Per entry point: its faults, numbered; one line for the base call and for each single fault; and for
the pairs of faults one line per first fault with one character per second fault, in the numbered order, for each build. Run it at two
commits and diff the outputs to show that a change to the rule headers (csrc/hm_*_rules.h) or to either build's use of them left every answer
as it was:

    python tools/entry_rules_sweep.py > this.txt
    HDRMERGE_LIB=<other>/libhdrmerge.so HDRMERGE_HOST_LIB=<other>/libhdrmerge_host.so python tools/entry_rules_sweep.py > other.txt

A status is printed as one character: 0 HM_OK, 1 HM_EINVAL, 2 HM_EUNSUPPORTED, 3 HM_EALIGN, 6 HM_ESHAPE; `-` the case is not sent to that
build (a valid call is never given to the device build, a valid call too large to run not to the host build, and nothing goes to the
device build on a machine with a GPU); `.` the two faults are no case of the sweep (they change the same argument, or their codes are equal).
"""
import importlib.util
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
spec = importlib.util.spec_from_file_location("entry_rules_cases", ROOT / "tests" / "test_entry_rules_host.py")
sweep = importlib.util.module_from_spec(spec)
spec.loader.exec_module(sweep)

from camera_linearity_amd import _native as nat  # noqa: E402

got = {}
for cid, build, rc, _ in sweep.sweep(nat.hip_lib, nat.host_lib()):
    got[cid, build] = "-" if rc is None else str(-rc)


def row(cids):
    return "  ".join(f"{b} {''.join(got.get((c, b), '.') for c in cids)}" for b in ("device", "host"))


for e in sweep.ENTRIES:
    names = [f.name for f in e.faults]
    print(f"== {e.cid} ({e.fn}): " + ", ".join(f"{i} {n}" for i, n in enumerate(names)))
    for n in ["base"] + names:
        print(f"{n:<34} {row([f'{e.cid}/{n}'])}")
    for i, n in enumerate(names[:-1]):
        print(f"{n + ' &':<34} {row([f'{e.cid}/{n} & {m}' for m in names[i + 1:]])}")
assert len(got) == 2 * sum(1 for _ in sweep.cases())
