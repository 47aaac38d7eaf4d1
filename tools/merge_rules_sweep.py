#!/usr/bin/env python3
"""Print the argument-rule sweep of tests/test_merge_rules_host.py, one line per case: status, kernels named and algorithmic bytes of the
device build (dry: no GPU needed) and of the host build. Run it at two commits and diff the outputs to show that a change to the rules
(csrc/hm_merge_rules.h) or to either build's use of them left every answer as it was:

    python tools/merge_rules_sweep.py > this.txt
    HDRMERGE_LIB=<other>/libhdrmerge.so HDRMERGE_HOST_LIB=<other>/libhdrmerge_host.so python tools/merge_rules_sweep.py > other.txt
"""
import importlib.util
import pathlib
import sys

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
spec = importlib.util.spec_from_file_location("merge_rules_cases", ROOT / "tests" / "test_merge_rules_host.py")
sweep = importlib.util.module_from_spec(spec)
spec.loader.exec_module(sweep)

from camera_linearity_amd import _native as nat  # noqa: E402

for cid, call in sweep.cases():
    for which, lib in (("device", nat.hip_lib), ("host", nat.host_lib())):
        rc, names, nbytes = call.probe(lib)
        print(f"{cid:<58} {which:<6} rc={rc:<3} bytes={nbytes:<10} {names}")
