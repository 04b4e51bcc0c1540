"""development aid: two timeline figures of a batched SLAM run from a per-dispatch kernel trace (`rocprofv3 --kernel-trace
--output-format csv -- python bench.py --full --no-extra --cpu-sample 0 --steps 10 --warmup 2`; no counters in the same run).

A call is one run_staged: its detection begins with k_threshold and ends with k_pose; its work on the EKF stream is --windows
consecutive k_ekf_win_step dispatches (the windows of a call: 10 for a lap of the headline scene) with the k_ekf_win_next between
them.  Detections and EKF groups are matched from the end of the trace, where every call is a full lap.
Printed, over the calls of the trace (medians; the first calls are left out with --skip):
  1. the idle time on the EKF stream between the last EKF kernel of one call and the first of the next (how far the host's
     wait / plan / enqueue and the call's detection stand behind the chain);
  2. the start of each call's k_threshold relative to the end of the EKF work two calls earlier (the slots it reuses): positive =
     the detection began after that work had ended (it waited for it, or had nothing else to wait for), negative = it ran beside it.

usage: python scripts/trace_call_gaps.py <kernel_trace.csv> [--skip N] [--windows W]"""
import csv
import statistics
import sys


def main():
    path = sys.argv[1]
    skip = int(sys.argv[sys.argv.index("--skip") + 1]) if "--skip" in sys.argv else 4
    rows = []
    with open(path, newline="") as f:
        for r in csv.DictReader(f):
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    short = lambda n: n.split("(")[0].split("<")[0].split("::")[-1].split()[-1]  # noqa: E731
    # detections: from a k_threshold to the next k_pose
    det = []
    for s, e, n in rows:
        k = short(n)
        if k == "k_threshold":
            det.append([s, None])
        elif k.startswith("k_pose") and det and det[-1][1] is None:
            det[-1][1] = e
    det = [d for d in det if d[1] is not None]
    W = int(sys.argv[sys.argv.index("--windows") + 1]) if "--windows" in sys.argv else 10
    chain = [(s, e, short(n)) for s, e, n in rows if short(n) in ("k_ekf_win_step", "k_ekf_win_next")]
    groups, cur, nstep = [], [], 0
    for s, e, k in reversed(chain):                        # from the end: groups of W step dispatches
        cur.append((s, e))
        if k == "k_ekf_win_step":
            nstep += 1
            if nstep == W:
                groups.append(cur)
                cur, nstep = [], 0
    groups.reverse()
    n = min(len(groups), len(det))
    calls = []
    for (ds, de), g in zip(det[-n:], groups[-n:]):
        calls.append(dict(det_start=ds, det_end=de, ekf_start=min(s for s, _ in g), ekf_end=max(e for _, e in g)))
    use = calls[skip:]
    if len(use) < 4:
        print(f"{len(calls)} calls with EKF work in the trace: too few after skipping {skip}")
        return
    idle = [(b["ekf_start"] - a["ekf_end"]) / 1e3 for a, b in zip(use, use[1:])]
    lead = [(c["det_start"] - a["ekf_end"]) / 1e3 for a, c in zip(use, use[2:])]
    span = [(b["ekf_start"] - a["ekf_start"]) / 1e3 for a, b in zip(use, use[1:])]
    det_len = [(c["det_end"] - c["det_start"]) / 1e3 for c in use]
    ekf_len = [(c["ekf_end"] - c["ekf_start"]) / 1e3 for c in use]
    med = statistics.median
    print(f"{len(use)} calls (of {len(calls)}; the first {skip} left out), microseconds, median (min .. max)")
    fmt = lambda v: f"{med(v):9.1f} ({min(v):.1f} .. {max(v):.1f})"  # noqa: E731
    print(f"call to call on the EKF stream (first EKF kernel to first EKF kernel):    {fmt(span)}")
    print(f"EKF work of a call, first kernel's start to last kernel's end:            {fmt(ekf_len)}")
    print(f"detection of a call, k_threshold's start to k_pose's end:                 {fmt(det_len)}")
    print(f"1. EKF stream idle between the last EKF kernel of a call and the next's:  {fmt(idle)}")
    print(f"2. k_threshold's start after the end of the EKF work two calls earlier:   {fmt(lead)}")


if __name__ == "__main__":
    main()
