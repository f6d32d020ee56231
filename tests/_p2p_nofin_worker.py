"""bench.py with the N-rank level finalisation as its own launch
(HipTreeBuilder.FUSE_FIN = False); same command line as bench.py."""
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from h2omx.models.tree.engine import HipTreeBuilder  # noqa: E402

HipTreeBuilder.FUSE_FIN = False
sys.argv[0] = os.path.join(ROOT, "bench.py")
runpy.run_path(sys.argv[0], run_name="__main__")
