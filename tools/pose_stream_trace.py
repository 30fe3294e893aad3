#!/usr/bin/env python
"""Diagnostic: the pose stream of the C++ frame loop in a rocprofv3 --kernel-trace CSV (`rocprofv3 --kernel-trace --stats --output-format csv
-d DIR -- tools/cxx/frame_loop.bin <workload> 300 30 0 2`).  Pose stream = the queue of k_intracam; a frame = k_intracam to k_intracam, the
last N.  Per kernel of that queue: launches per frame, median / mean / max duration, total per frame; the stream's busy time and span per
frame.  For the kernels named with --watch: the gap to the previous kernel of the queue, and which kernels of the OTHER queues run inside
[previous kernel's end, this kernel's end] -- what a launch that waits for room would be waiting for.
Usage: pose_stream_trace.py LABEL=kernel_trace.csv [LABEL=...] [--frames 300] [--watch k_revisit_rounds,k_map_points_classify]"""
import csv
import statistics as st
import sys
from collections import Counter, defaultdict


def short(n):
    return n.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0].split("<")[0]


def load(path):
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((short(r["Kernel_Name"]), int(r["Queue_Id"]), int(r["Start_Timestamp"]), int(r["End_Timestamp"])))
    rows.sort(key=lambda r: r[2])
    return rows


def report(label, rows, n_frames, watch):
    q_pose = Counter(q for n, q, s, e in rows if n == "k_intracam").most_common(1)[0][0]
    pose = [r for r in rows if r[1] == q_pose]
    other = [r for r in rows if r[1] != q_pose]
    marks = [i for i, r in enumerate(pose) if r[0] == "k_intracam"]
    marks = marks[-(n_frames + 1):]
    nf = len(marks) - 1
    per = defaultdict(list)
    busy, span, launches = [], [], []
    for a, b in zip(marks[:-1], marks[1:]):
        fr = pose[a:b]
        busy.append(sum(e - s for _, _, s, e in fr) / 1e3)
        span.append((pose[b][2] - pose[a][2]) / 1e3)
        launches.append(len(fr))
        for n, _, s, e in fr:
            per[n].append((e - s) / 1e3)
    print(f"== {label}: queue {q_pose}, {nf} frames; pose-stream launches per frame: median {st.median(launches):.1f} (min {min(launches)}, max {max(launches)}); "
          f"busy {st.mean(busy):.1f} us/frame, span mean {st.mean(span):.1f} median {st.median(span):.1f} us/frame")
    for n, d in sorted(per.items(), key=lambda kv: -sum(kv[1])):
        print(f"   {n:34s} {len(d) / nf:5.2f}/frame  median {st.median(d):7.2f} us  mean {st.mean(d):7.2f}  max {max(d):8.2f}  total/frame {sum(d) / nf:7.2f}")
    lo, hi = pose[marks[0]][2], pose[marks[-1]][2]
    oth = [r for r in other if r[3] >= lo and r[2] <= hi]
    for w in watch:
        idx = [i for i in range(marks[0] + 1, marks[-1]) if pose[i][0] == w]
        if not idx:
            continue
        durs = [(pose[i][3] - pose[i][2]) / 1e3 for i in idx]
        med = st.median(durs)
        for name, sel in (("at or below the median duration", [i for i, d in zip(idx, durs) if d <= med]), ("above it", [i for i, d in zip(idx, durs) if d > med])):
            if not sel:
                continue
            gaps = [(pose[i][2] - pose[i - 1][3]) / 1e3 for i in sel]
            ov, ov_us, none, j0 = Counter(), Counter(), 0, 0
            for i in sel:
                t0, t1 = pose[i - 1][3], pose[i][3]
                while j0 < len(oth) and oth[j0][3] < t0 - 2_000_000:
                    j0 += 1
                seen = set()
                for j in range(j0, len(oth)):
                    n, _, s, e = oth[j]
                    if s > t1:
                        break
                    if e > t0:
                        seen.add(n)
                        ov_us[n] += (min(e, t1) - max(s, t0)) / 1e3
                none += not seen
                ov.update(seen)
            print(f"   {w}, {len(sel)} launches {name} ({med:.2f} us): duration median {st.median([(pose[i][3] - pose[i][2]) / 1e3 for i in sel]):.2f} us, gap to the "
                  f"previous kernel median {st.median(gaps):.2f} mean {st.mean(gaps):.2f} us; alone on the device in {none}; other queues' kernels inside "
                  f"[previous end, end]:")
            for n, c in ov.most_common(8):
                print(f"      {n:34s} in {c:4d} of {len(sel)}  ({ov_us[n] / c:6.1f} us overlap each)")


def main():
    args = sys.argv[1:]
    n_frames, watch, files = 300, ["k_revisit_rounds", "k_map_points_classify"], []
    while args:
        a = args.pop(0)
        if a == "--frames":
            n_frames = int(args.pop(0))
        elif a == "--watch":
            watch = args.pop(0).split(",")
        else:
            files.append(a.split("=", 1) if "=" in a else (a, a))
    for label, path in files:
        report(label, load(path), n_frames, watch)


if __name__ == "__main__":
    main()
