"""The tail of the headline's steps from a rocprofv3 --kernel-trace CSV: what runs behind a step's last fused scan launch.
bench.py launches a 16-byte fill_kernel right before and right after its timed region (tools/launch_rows.py); a step of the
timed region begins with a fused scan launch and ends where the next step's first one begins (the last step: at the marker).
Prints, over all timed steps, the time from the end of a step's last fused launch to the step's end (median, min, max), how long
the runtime's copy kernels (__amd_rocclr_copyBuffer) run in that tail and how much of that lies under replay_* / stitch_* kernels,
and then the last step's tail row by row.
usage: tools/tail_timeline.py KERNEL_TRACE.csv [LAUNCHES_PER_STEP=2] > profiles/TAG_tail.txt"""
import csv
import statistics
import sys

rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
per_step = int(sys.argv[2]) if len(sys.argv) > 2 else 2
ev = [(int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"].split("(")[0].replace("void ", "").replace("sx::", "")) for r in rows]
fills = [i for i, e in enumerate(ev) if "fill_kernel" in e[2]]
m0, m1 = fills[-2], fills[-1]
timed = ev[m0 + 1:m1]
scans = [i for i, e in enumerate(timed) if e[2].startswith("scan_kernel_fused")]
assert scans and len(scans) % per_step == 0, (len(scans), per_step)
steps = len(scans) // per_step


def overlap(a, group):
    """nanoseconds of [a0, a1) covered by the union of the intervals in `group`"""
    cut = sorted((max(a[0], s), min(a[1], e)) for s, e, _ in group if s < a[1] and e > a[0])
    total, at = 0, a[0]
    for s, e in cut:
        s = max(s, at)
        if e > s:
            total += e - s
            at = e
    return total


tails, copies, hidden = [], [], []
for k in range(steps):
    last = timed[scans[k * per_step + per_step - 1]]
    end = timed[scans[(k + 1) * per_step]][0] if k + 1 < steps else ev[m1][0]
    behind = [e for e in timed if e[0] >= last[1] and e[0] < end]
    tails.append((end - last[1]) / 1e6)
    cp = [e for e in behind if "copyBuffer" in e[2]]
    rp = [e for e in behind if e[2].startswith(("replay_", "stitch_"))]
    copies.append(sum(e[1] - e[0] for e in cp) / 1e6)
    hidden.append(sum(overlap(e, rp) for e in cp) / 1e6)
print(f"timed steps: {steps}, fused launches per step: {per_step}")
print(f"end of the last fused launch -> end of the step: median {statistics.median(tails):.3f} ms, min {min(tails):.3f}, max {max(tails):.3f}")
print(f"copyBuffer kernels in that tail: median {statistics.median(copies):.3f} ms per step, of which under replay_* / stitch_* kernels: "
      f"median {statistics.median(hidden):.3f} ms")
print("the last step's tail (offset from the end of its last fused launch, duration, kernel; rows of 5 us and more):")
last = timed[scans[-1]]
for s, e, n in timed:
    if s >= last[1] and e - s >= 5000:
        print(f"{(s - last[1]) / 1e6:9.3f} ms  +{(e - s) / 1e6:7.3f} ms  {n[-70:]}")
