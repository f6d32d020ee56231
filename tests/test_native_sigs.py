"""The ctypes signature strings of ``h2omx.ops`` against the C prototypes they
bind: a swapped or missing letter is a wrong argument on the GPU, not a
failing test, so every bound name must match its ``H2OMX_API`` prototype."""
from __future__ import annotations

import glob
import os
import re

from h2omx import ops

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "h2omx", "csrc")
PROTO = re.compile(r"^H2OMX_API\s+[\w:\s*]+?\b(h2omx_\w+)\s*\(([^)]*)\)", re.M)
SCALARS = {"hipStream_t": "S", "int64_t": "L", "long long": "L", "int": "I", "uint32_t": "U", "unsigned int": "U",
           "float": "F", "double": "D"}


def _letter(param: str, where: str) -> str:
    if "*" in param:
        return "P"
    words = [w for w in param.split() if w != "const"]
    ctype = " ".join(words[:-1])   # "<type> <name>"
    assert ctype in SCALARS, f"{where}: cannot map parameter {param!r}"
    return SCALARS[ctype]


def _prototypes() -> dict[str, str]:
    protos = {}
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip"))):
        with open(path) as fh:
            src = fh.read()
        for m in PROTO.finditer(src):
            name, params = m.group(1), m.group(2).strip()
            assert name not in protos, f"{name}: defined twice"
            plist = [] if params in ("", "void") else params.split(",")
            protos[name] = "".join(_letter(p, name) for p in plist)
    return protos


def test_binding_strings_match_prototypes():
    protos = _prototypes()
    bound = 0
    for table in (ops.TREE_SIGS, ops.DENSE_SIGS, ops.METRICS_SIGS, ops.EXPLAIN_SIGS, ops.P2P_SIGS):
        for name, sig in table.items():
            assert name in protos, f"{name}: bound but no H2OMX_API prototype in csrc/*.hip"
            assert protos[name] == sig, f"{name}: prototype is {protos[name]!r}, binding says {sig!r}"
            bound += 1
    assert bound > 100   # the parser found the sources
