"""snk_ba_set_problems_dev in a child process: SNK_BA_CHECK_LISTS and SNK_DEBUG_POISON (like every switch of the library) are read once,
so `python handover_children.py OUT.npz` loads the 17-problem batch and the constraint batch of tests/handover_cases.py from device rows --
under the switches the parent set: the host builder runs beside the device stage and every array is compared element for element, on
scratch that was filled with a pattern -- solves them, hands the 17-problem batch over a second time on the same handle, and writes every
result as bytes.  The parent (tests/test_ba_handover_dev_gpu.py) compares with the host-array hand-over of its own, unswitched process."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np

TESTS = Path(__file__).resolve().parent
for p in (str(TESTS.parent), str(TESTS)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out):
    import handover_cases as HC
    import handover_numpy as M

    res = {}
    o17, orpc = M.pad_rows(HC.unequal_batch(17), dict(pt_cap=100, img_cap=16, obs_cap=700)), M.pad_rows(HC.constraint_batch())
    ba, keep = HC.load_dev(o17)
    for k, b in HC.collect(ba, 17):
        res[f"first_{k}"] = np.frombuffer(b, np.uint8)
    ba, keep2 = HC.load_dev(orpc, ba=ba)  # another batch on the same handle
    for k, b in HC.collect(ba, 3):
        res[f"rpc_{k}"] = np.frombuffer(b, np.uint8)
    ba, keep3 = HC.load_dev(o17, ba=ba)  # and the first one again
    for k, b in HC.collect(ba, 17):
        res[f"again_{k}"] = np.frombuffer(b, np.uint8)
    ba.close()
    np.savez(out, **res)


def run_child(out, **switches):
    r = subprocess.run([sys.executable, str(Path(__file__).resolve()), str(out)], env=dict(os.environ, **switches), capture_output=True, text=True,
                       cwd=str(TESTS.parent), timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    return r


if __name__ == "__main__":
    main(sys.argv[1])
