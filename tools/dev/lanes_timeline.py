"""Per-stream timeline of one timed bench frame from a rocprofv3 kernel trace (tools/dev/timeline.sh, or `rocprofv3 --kernel-trace --output-format csv`):
the launches of the two lanes, and how long k_shade / k_trace of one lane overlap those of the other.  usage: lanes_timeline.py t_kernel_trace.csv [frame]"""
import csv, sys
rows = list(csv.DictReader(open(sys.argv[1])))
ev = []
for r in rows:
    n = r["Kernel_Name"]
    short = n.split("(")[0].replace("void ", "")
    if "k_" in short: short = "k_" + short.split("k_", 1)[1]
    ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), short[:26], r["Stream_Id"], r["Queue_Id"]))
ev.sort()
# frames of the timed loop: they start at a k_raygen that follows a k_resolve
frames, cur = [], []
for e in ev:
    if e[2].startswith("k_raygen") and cur and any(x[2].startswith("k_resolve") for x in cur):
        frames.append(cur); cur = []
    cur.append(e)
frames.append(cur)
which = int(sys.argv[2]) if len(sys.argv) > 2 else 2
f = frames[which]
t0 = f[0][0]
streams = sorted(set(e[3] for e in f), key=int)
print("frame %d of %d; span %.3f ms; streams %s" % (which, len(frames), (max(e[1] for e in f) - t0) / 1e6, streams))
for s, e, n, st, q in f:
    if n.startswith(("k_trace", "k_shade", "k_raygen", "k_accum")):
        print("  stream %-3s %-26s %8.3f -> %8.3f  (%6.3f ms)" % (st, n, (s - t0) / 1e6, (e - t0) / 1e6, (e - s) / 1e6))
# overlap of k_shade on one stream with k_trace on another, and of the two streams' k_shade with each other
def iv(pred, st): return [(s, e) for s, e, n, x, q in f if pred(n) and x == st]
def ov(a, b): return sum(max(0, min(e1, e2) - max(s1, s2)) for s1, e1 in a for s2, e2 in b) / 1e6
if len(streams) >= 2:
    lanes = [x for x in streams if iv(lambda n: n.startswith("k_shade"), x)]
    if len(lanes) >= 2:
        a, b = lanes[:2]
        sh = lambda n: n.startswith("k_shade"); tr = lambda n: n.startswith("k_trace")
        print("k_shade total: lane %s %.3f ms, lane %s %.3f ms" % (a, sum(e - s for s, e in iv(sh, a)) / 1e6, b, sum(e - s for s, e in iv(sh, b)) / 1e6))
        print("overlap k_shade(%s) x k_shade(%s): %.3f ms" % (a, b, ov(iv(sh, a), iv(sh, b))))
        print("overlap k_shade(%s) x k_trace(%s): %.3f ms; k_shade(%s) x k_trace(%s): %.3f ms" % (a, b, ov(iv(sh, a), iv(tr, b)), b, a, ov(iv(sh, b), iv(tr, a))))
        print("overlap k_trace(%s) x k_trace(%s): %.3f ms" % (a, b, ov(iv(tr, a), iv(tr, b))))
