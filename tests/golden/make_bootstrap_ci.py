#!/usr/bin/env python3
"""Writes tests/golden/bootstrap_ci.json: the confidence-interval columns sylph_host_stats(no_ci=0, min_ani=0, k=31) gives for
tests/bootstrap_ref.py's oracle_shaped_vectors(), recorded from the library of the commit BEFORE the statistics were split in two
(libsylph_host.so built from that commit).  Usage: python tests/golden/make_bootstrap_ci.py /path/to/that/libsylph_host.so"""
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
from tests.bootstrap_ref import CI_FIELDS, HostStats, oracle_shaped_vectors   # noqa: E402

L = C.CDLL(os.path.abspath(sys.argv[1]))
L.sylph_host_stats.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_double, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(HostStats)]
rows = []
for covs, n_kmers in oracle_shaped_vectors():
    cv, out = np.ascontiguousarray(covs, dtype=np.uint32), HostStats()
    L.sylph_host_stats(cv.ctypes.data_as(C.c_void_p), len(cv), n_kmers, 31, 3.0, 0.0, 0, 0, 0, 0, C.byref(out))
    rows.append([int(out.passed), int(out.has_ci)] + [getattr(out, f).hex() for f in CI_FIELDS])
path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "bootstrap_ci.json")
json.dump({"fields": ["passed", "has_ci"] + list(CI_FIELDS), "note": "doubles as float.hex()", "rows": rows}, open(path, "w"), indent=0)
print(f"{len(rows)} rows, {sum(r[1] for r in rows)} with an interval -> {path}")
