"""Every byte rt_scene_commit writes on the device, against the digests frozen from an earlier
library (tests/golden/commit_digests.json; tests/commit_digest_cases.py says why and holds the
sequences): the four-wide nodes, leaf boxes, TLAS leaf boxes, bcoord and instance bounds after plain,
rebuilding and deforming commits, on two replicas."""
import json
import os
import sys
import time

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import commit_digest_cases as CD                                                 # noqa: E402

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "commit_digests.json")) as _fh:
    GOLDEN = json.load(_fh)


@pytest.mark.parametrize("name", list(CD.CASES))
def test_commit_writes_the_frozen_bytes_on_both_replicas(name):
    t0 = time.time()
    got = CD.run(name, [0, 0])
    print(f"{name}: {time.time() - t0:.2f} s")
    want = GOLDEN["cases"][name]
    assert sorted(got) == sorted(want)
    for label, per_replica in got.items():
        assert per_replica == [want[label]] * 2, f"{name} / {label}: {per_replica} != {want[label]}"
