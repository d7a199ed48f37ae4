#!/usr/bin/env python3
"""Freeze what rt_scene_commit writes on the device (test infrastructure; run by hand on a GPU
machine like make_frame_golden.py, with the library of the commit whose bytes are to be kept - not
with the code under test).

Every case of tests/commit_digest_cases.py runs twice on two replicas of device 0.  A case is
written only if both runs and both replicas give the same digests; one that does not is not
deterministic, cannot serve, and is named on stdout.  commit_digests.json then holds
  lib_sha256_16   of the library that produced the digests
  cases           case -> label -> SHA-256 (commit_digest_cases.digest)
  python tests/golden/make_commit_golden.py [output.json]
"""
import hashlib
import json
import os
import sys
import traceback

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import myraytracer_amd as M  # noqa: E402

import commit_digest_cases as CD  # noqa: E402


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "commit_digests.json")
    M.load_library()
    with open(M.engine.LIB_PATH, "rb") as fh:
        rec = {"lib_sha256_16": hashlib.sha256(fh.read()).hexdigest()[:16], "cases": {}}
    dropped = []
    for name in CD.CASES:
        try:
            runs = [CD.run(name, [0, 0]) for _ in range(2)]
        except Exception:
            traceback.print_exc()
            dropped.append(name)
            continue
        same = runs[0] == runs[1] and all(len(set(v)) == 1 for v in runs[0].values())
        print(f"{name}: {'deterministic' if same else 'NOT deterministic, dropped'}", flush=True)
        for label, v in runs[0].items():
            print(f"    {label}: {v[0]}")
        if same:
            rec["cases"][name] = {label: v[0] for label, v in runs[0].items()}
        else:
            dropped.append(name)
    with open(out_path, "w") as fh:
        json.dump(rec, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out_path, "; dropped:", dropped or "none")
    return 1 if dropped else 0


if __name__ == "__main__":
    sys.exit(main())
