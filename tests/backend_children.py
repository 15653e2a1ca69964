"""The back-end seams of tests/backend_cases.py in a child process: SNK_DEBUG_POISON (like every switch of the library) is read once, so
`python backend_children.py GROUP OUT.npz` runs the seams of one group of backend_cases.GROUPS on handles of their own, on cases 0, 1, 2,
and writes every result as bytes.  The parent (tests/test_backend_scratch_gpu.py) compares with the unpoisoned results of its own
process."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

TESTS = Path(__file__).resolve().parent
for p in (str(TESTS.parent), str(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(group, out):
    import backend_cases as BC

    res = {}
    for name in BC.GROUPS[group]:
        for k, b in enumerate(BC.solo(name)):
            res[f"{name}_{k}"] = np.frombuffer(b, np.uint8)
    np.savez(out, **res)


def run_child(group, out, **switches):
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), group, str(out)], env=dict(os.environ, **switches), capture_output=True,
                       text=True, cwd=str(TESTS.parent), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
