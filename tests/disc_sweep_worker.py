"""One rank of the shared-card rehearsal of the discrepancy sweep (tests/test_gpu_discrepancy_sweep.py):
`lemon_amd.discrepancy_baseline.main` on a disc_* fixture's planted model / data, alone or under WORLD_SIZE=2 with
LEMON_DIST_BACKEND=gloo (RCCL needs distinct devices; both ranks use cuda:0).
argv: <fixture method> <output dir> <data dir> [further CLI flags]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class _Patch:
    def setattr(self, obj, name, value):
        setattr(obj, name, value)


def main():
    method, out_dir, data_dir = sys.argv[1:4]
    from pathlib import Path
    from types import SimpleNamespace

    import numpy as np

    from tests import planted
    from lemon_amd.discrepancy_baseline import main as run
    fx = np.load(os.path.join(ROOT, "tests", "golden", f"disc_{method}.npz"))
    case = SimpleNamespace(fx=fx, is_caption=False, dataset="cifar10")
    extra = planted.install(case, _Patch(), Path(data_dir) / f"rank{os.environ.get('RANK', '0')}")
    return run(["--output_dir", out_dir] + json.loads(str(fx["argv"])) + extra + sys.argv[4:])


if __name__ == "__main__":
    sys.exit(main())
