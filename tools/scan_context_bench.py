"""Time Scan Context place recognition: the descriptor of the 200k-point synthetic benchmark source (pcr_scan_context at the defaults), the
all-pairs distance block of 1024 x 1024 descriptors (pcr_scan_context_distance; rolled and perturbed copies of the golden scans' descriptors, so
that columns are filled as a LiDAR fills them), and ScanContextDatabase.detect_loop_closures on those 1024 rows.  Device events around whole
calls, one warm-up call, the median of `reps` with the spread, nothing else in flight.
usage: scan_context_bench.py [reps]"""
import glob, importlib, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
P = importlib.import_module("point-cloud-registration-with-global-refinement_amd")
syn = importlib.import_module("point-cloud-registration-with-global-refinement_amd.synthetic")
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
R, S, N = 20, 60, 1024


def timed(name, fn, work=None):
    out = fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); out = fn(); b.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(b))
    med = float(np.median(ts))
    rate = f", {work / med * 1e-6:.2f} G multiply-adds/s" if work else ""
    print(f"{name}: median {med:.3f} ms (min {min(ts):.3f}, max {max(ts):.3f}, {reps} calls){rate}", flush=True)
    return out


cloud = torch.from_numpy(np.ascontiguousarray(np.asarray(syn.make_pair(200000, index=0).source, np.float32))).cuda()
print(f"== synthetic cloud: n = {cloud.shape[0]}", flush=True)
desc, info = P.scan_context(cloud, return_info=True)
print(f"rows {info}, {int((desc != 0).sum())} of {R * S} cells occupied", flush=True)
timed("scan_context (no info: asynchronous)", lambda: P.scan_context(cloud))
timed("scan_context (with the row counts: one read-back)", lambda: P.scan_context(cloud, return_info=True))

scans = []
for f in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "nclt_pair_*.npz"))):
    d = np.load(f)
    scans += [d["source"], d["target"]]
base = torch.stack([P.scan_context(c) for c in scans])
rng = np.random.default_rng(1)
rows = torch.stack([torch.roll(base[k % len(scans)], int(rng.integers(S)), dims=1) for k in range(N)])
rows = (rows * torch.from_numpy(rng.uniform(0.9, 1.1, (N, R, S)).astype(np.float32)).cuda()).contiguous()
print(f"== {N} descriptors of {R} x {S}", flush=True)
timed(f"scan_context_distance {N} x {N}", lambda: P.scan_context_distance(rows, rows), work=float(N) * N * S * S * R)
timed(f"scan_context_distance 1 x {N}", lambda: P.scan_context_distance(rows[:1], rows), work=float(N) * S * S * R)
with P.ScanContextDatabase() as db:
    db._reserve(N); db._store[:N] = rows; db._n = N
    out = timed(f"detect_loop_closures(0.4, exclude_recent=50) on {N} rows", lambda: db.detect_loop_closures(0.4, exclude_recent=50))
    print(f"closures found: {len(out[0])}", flush=True)
