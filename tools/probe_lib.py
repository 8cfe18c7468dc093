"""The library switch of the probes: SDENG_LIB = another build of libsdeng.so with the same ABI (python -m sde_sampler_lrds_amd.build with
SDENG_OUT=...), loaded instead of the in-tree one.  As in tools/probe_ab.py the path is set before the library's first use, and an A/B runs
one fresh process per library."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def select():
    """Point the binding at SDENG_LIB when it is set -> the name of the library in use, for the probe's header line."""
    from sde_sampler_lrds_amd import _lib
    alt = os.environ.get("SDENG_LIB")
    if alt:
        _lib.LIB_PATH = os.path.abspath(alt)
    return _lib.LIB_PATH
