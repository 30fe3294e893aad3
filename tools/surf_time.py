#!/usr/bin/env python
"""Stand-alone timing of the SURF stage: 8 cameras 640 x 480 (one blob texture, rolled by a different offset per camera),
4 octaves, 2 octave layers, dim 64, threshold 100.  Timed, HIP events around back-to-back calls after a warm-up, the median of 7 blocks with
their spread, the entry points that stop after a stage -- so a stage is the difference of two neighbours:
  integral   cs_surf_integral_dev
  layers     cs_surf_layers_dev  - integral      (k_surf_response)
  lists      cs_surf_detect_dev  - layers        (maxima, scan, scatter, padding)
  describe   cs_surf_run_dev     - detect        (orientation and descriptors; upright: descriptors alone)
and the whole call.  Next to them the numpy restatement (tests/surf_ref.py) of ONE camera on the CPU, the key-point counts, and the
response kernel's traffic: 28 integral reads of 4 bytes per sample, 9 bytes written.  Nothing is gated.
--keep first | strongest (default first): the handle's choice beyond max_pts; --max-pts N (default 2048): with strongest, a value below the
cameras' maxima makes the select run (its cost is `lists` against the same run with --keep first)."""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
import coslam_amd
from tests import surf_ref as R
from tests import surf_scenes as S

N_CAMS, W, H, MAX_PTS, THR = 8, 640, 480, 2048, 100.0
KEEP = sys.argv[sys.argv.index("--keep") + 1] if "--keep" in sys.argv else "first"
if "--max-pts" in sys.argv:
    MAX_PTS = int(sys.argv[sys.argv.index("--max-pts") + 1])
KW = dict(keep=KEEP) if KEEP != "first" else {}          # (no keyword: the tool also times an older build of the package)
print(f"keep = {KEEP}, max_pts = {MAX_PTS}")


def timed(run, reps=5, blocks=7, warm=2):
    for _ in range(warm): run()
    torch.cuda.synchronize()
    out = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps): run()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / reps * 1e3)
    return np.median(out), min(out), max(out)


base = S.texture(W, H, 0)
imgs = [np.ascontiguousarray(np.roll(base, (37 * c, 53 * c), axis=(0, 1))) for c in range(N_CAMS)]
dev = [torch.as_tensor(im, device="cuda") for im in imgs]
t0 = time.perf_counter()
ref = R.run(imgs[0], THR)
t_ref = time.perf_counter() - t0
t0 = time.perf_counter()
R.layer_maps(R.integral(imgs[0]))
t_maps = time.perf_counter() - t0
print(f"numpy restatement, 1 camera {W} x {H}: {t_ref * 1e3:.0f} ms (integral + layer maps {t_maps * 1e3:.0f} ms): {ref['count']} key points, "
      f"per octave {np.bincount(ref['octave'], minlength=4).tolist()}")
for upright in (False, True):
    sf = coslam_amd.Surf(N_CAMS, W, H, MAX_PTS, **KW)
    a = timed(lambda: sf.integral(dev))
    b = timed(lambda: sf.layers(dev))
    c = timed(lambda: sf.detect(dev, THR))
    d = timed(lambda: sf.enqueue(dev, THR, upright=upright))
    cnt, ovf = sf.counts()
    got = sf.keypoints(0)
    same = ref["count"] == cnt[0] + ovf[0] and (ovf[0] > 0 or np.array_equal(got["cell"], ref["cell"]))
    print(f"upright {int(upright)}: integral {a[0]:7.1f} us [{a[1]:.1f} .. {a[2]:.1f}]  layers {b[0] - a[0]:7.1f} us (with integral {b[0]:.1f} [{b[1]:.1f} .. {b[2]:.1f}])  "
          f"lists {c[0] - b[0]:7.1f} us (detect {c[0]:.1f} [{c[1]:.1f} .. {c[2]:.1f}])  describe {d[0] - c[0]:7.1f} us  whole {d[0]:7.1f} us [{d[1]:.1f} .. {d[2]:.1f}]")
    print(f"           key points per camera {cnt.tolist()}, overflow {ovf.tolist()}; camera 0 is the restatement's list: {bool(same)}")
    if not upright:
        samples = N_CAMS * sf.buf.mapElems
        t_resp = (b[0] - a[0]) * 1e-6
        print(f"           response kernel: {samples} samples, {samples * 112 / 1e9:.2f} GB of integral reads (cache), {samples * 9 / 1e6:.0f} MB written: "
              f"{samples * 112 / t_resp / 1e12:.2f} TB/s read, {samples * 9 / t_resp / 1e12:.3f} TB/s written (this one run); maps {samples * 9 / 1e6:.0f} MB, "
              f"integral images {N_CAMS * (W + 1) * (H + 1) * 4 / 1e6:.1f} MB")
    sf.close()
