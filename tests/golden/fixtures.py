"""The committed fixtures tests/golden/*_golden.npz as data: which maker produces each one, from which binaries under oracle/_ref/
(oracle/Makefile builds them where the reference tree exists), and how a regenerated copy is compared with the committed file.

    python tests/golden/make_golden.py [names...]      writes the named fixtures (all of them without names)
    tests/test_oracle_cpu.py                           regenerates every one in memory and compares (nothing is written)

compare:  "bytes"       same keys, same dtypes, same bytes
          "export_ids"  the same after every MapPoint::id has been replaced by its index in `ptId` (canonical_export_ids)
"""
import importlib
import os
import re
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref")

Fixture = namedtuple("Fixture", "name module function args binaries compare")


def _f(name, module, function, args=(), binaries=(), compare="bytes"):
    return Fixture(name, module, function, tuple(args), tuple(binaries), compare)


FIXTURES = [
    _f("pose", "make_golden", "pose_cases", binaries=["libintracam_ref.so"]),
    _f("klt", "make_golden", "klt_cases"),
    _f("ba", "make_golden", "ba_case"),
    _f("register", "make_golden", "register_case", binaries=["ref_register_test"]),
    _f("ncc", "make_golden", "ncc_case", binaries=["ref_ncc_test"]),
    _f("posegraph", "make_golden", "posegraph_case", binaries=["ref_posegraph_test"]),
    _f("export", "make_golden", "export_case", binaries=["ref_export_test"], compare="export_ids"),
    _f("intercam", "make_golden", "intercam_case", binaries=["ref_intercam_test"]),
    _f("mergability", "make_golden", "mergability_case", binaries=["ref_mergability_test"]),
    _f("mergability_long", "make_golden", "mergability_long_case", binaries=["ref_mergability_test"]),
    _f("update_points", "make_golden", "update_points_case", binaries=["ref_update_points_test"]),
    _f("update_points_relink", "make_golden", "update_points_relink_case", binaries=["ref_update_points_test"]),
    _f("update_points_wide", "make_golden", "update_points_case", ["golden_wide"], ["ref_update_points_test"]),
    _f("update_points_wide_relink", "make_golden", "update_points_relink_case", ["golden_wide_relink"], ["ref_update_points_test"]),
    _f("intracam_newpts", "make_golden", "intracam_newpts_case", binaries=["ref_intracam_newpts_test"]),
    _f("keyframe", "make_golden", "keyframe_case", binaries=["ref_keyframe_test"]),
    _f("classify", "make_golden", "classify_case", binaries=["ref_classify_test"]),
    _f("classify_relink", "make_golden", "classify_relink_case", binaries=["ref_classify_test"]),
    _f("classify_wide", "make_golden", "classify_case", ["golden_wide"], ["ref_classify_test"]),
    _f("classify_wide_relink", "make_golden", "classify_relink_case", ["golden_wide_relink"], ["ref_classify_test"]),
    _f("decide", "make_golden", "decide_case", binaries=["ref_decide_test"]),
    _f("decide_relink", "make_golden", "decide_relink_case", binaries=["ref_decide_test"]),
    _f("newpts", "make_golden", "newpts_case", binaries=["ref_newpts_test"]),
    _f("cgklt", "make_golden", "cgklt_cases", binaries=["libcgklt_ref.so"]),
    _f("mergegraph", "make_mergegraph_golden", "mergegraph_case", binaries=["ref_mergegraph_test"]),
    _f("mergeapply", "make_mergeapply_golden", "mergeapply_case", binaries=["ref_mergeapply_test"]),
    _f("mergeconstraints", "make_mergeconstraints_golden", "mergeconstraints_case", binaries=["ref_mergeconstraints_test"]),
    _f("mergematch", "make_mergematch_golden", "mergematch_case", binaries=["ref_mergematch_test"]),
]
BY_NAME = {f.name: f for f in FIXTURES}


def path(fx):
    return os.path.join(HERE, fx.name + "_golden.npz")


def missing_binaries(fx):
    return [b for b in fx.binaries if not os.path.exists(os.path.join(REF_DIR, b))]


def make(fx):
    """the fixture's arrays, made now: {key: array}"""
    return getattr(importlib.import_module("tests.golden." + fx.module), fx.function)(*fx.args)


class DriverPredatesMode(Exception):
    """A driver that was built from an older tree and kept (oracle/Makefile keeps a prebuilt _ref/ where it cannot rebuild it) does not
    know a newer mode: it answers with its usage line and status 2."""


def run_driver(driver, *args):
    """oracle/_ref/<driver> args...: returns its stdout; a status other than 0 raises."""
    exe = os.path.join(REF_DIR, driver)
    if not os.path.exists(exe):
        raise FileNotFoundError("oracle/_ref/%s missing: run `make -C oracle` where the reference tree exists" % driver)
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    if r.returncode == 2 and r.stderr.startswith("usage:"):
        raise DriverPredatesMode("oracle/_ref/%s predates its %s mode (kept from an older build; not rebuilt from this tree)" % (driver, args[0]))
    if r.returncode != 0:
        raise RuntimeError("oracle/_ref/%s %s: status %d\n%s" % (driver, args[0], r.returncode, r.stderr))
    return r.stdout


def driver_output(driver, mode):
    """the bytes of the one file `<driver> <mode> <file>` writes"""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "out.bin")
        run_driver(driver, mode, out)
        with open(out, "rb") as f:
            return f.read()


EXPORT_ID_TEXTS = ("file_mappts.txt", "file_0_featpts.txt", "file_1_featpts.txt")


def canonical_export_ids(arrays):
    """export_golden.npz's arrays with every MapPoint::id replaced by its index in `ptId`: in ptId itself, in c*_featId and in the
    three result files that print ids (every whitespace-separated token equal to a value of ptId).  Everything else is untouched."""
    out = {k: np.asarray(arrays[k]) for k in (arrays.files if hasattr(arrays, "files") else arrays)}
    ids = out["ptId"].ravel().tolist()
    index = {v: i for i, v in enumerate(ids)}
    assert len(index) == len(ids), "ptId holds a value twice"
    for k in out:
        if k == "ptId" or (k.startswith("c") and k.endswith("_featId")):
            a = out[k]
            out[k] = np.array([index.get(v, v) for v in a.ravel().tolist()], dtype=a.dtype).reshape(a.shape)
    token = {str(v).encode(): str(i).encode() for v, i in index.items()}
    for k in EXPORT_ID_TEXTS:
        out[k] = np.frombuffer(re.sub(rb"\S+", lambda m: token.get(m.group(), m.group()), out[k].tobytes()), dtype=np.uint8)
    return out
