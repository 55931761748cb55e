"""Dev tool: the nearest-neighbour kernels at the size of the pose dataset.

    python tools/knn_time.py [--rows 131072] [--dim 69] [--k 5] [--torch-reps 3]

knn_radii on `rows` x `dim` uniform rows, ball_query of 16 384 and of 64 of those rows against all of them; each timed
with event pairs, 1 warm-up and 5 timed runs, the median. For comparison torch.cdist + kthvalue / min in row chunks on
the same tensors, with the direct-difference distance (what the kernels compute; its radii on an eighth of the rows) and
with the matrix-multiply form (which cancels: see section 15.1). One JSON line on stdout, progress on stderr. Not part of any test and not read by bench.py."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from music2dance_amd import metrics

DEV = "cuda:0"
# rows of a torch chunk: the matrix-multiply form holds a 4096 x rows fp32 matrix; the direct form launches one workgroup
# of 256 threads per PAIR, and a launch may not exceed 2^32 threads
CHUNK = {"use_mm_for_euclid_dist": 4096, "donot_use_mm_for_euclid_dist": 64}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def say(*a):
    print(*a, file=sys.stderr, flush=True)


def torch_radii(X, k, mode, rows=None):
    """radii of the first `rows` rows (default: all) against all of X"""
    out = []
    for i in range(0, rows or X.shape[0], CHUNK[mode]):
        d = torch.cdist(X[i:i + CHUNK[mode]], X, compute_mode=mode)
        out.append(torch.kthvalue(d, k + 1, dim=1).values)        # the row itself is one of the k + 1 (by distance)
    return torch.cat(out) ** 2


def torch_query(Q, P, r, mode):
    cnt, nn = [], []
    for i in range(0, Q.shape[0], CHUNK[mode]):
        d = torch.cdist(Q[i:i + CHUNK[mode]], P, compute_mode=mode)
        cnt.append((d <= r[None, :]).sum(dim=1))
        nn.append(d.min(dim=1))
    return torch.cat(cnt), torch.cat([m.values for m in nn]), torch.cat([m.indices for m in nn])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--dim", type=int, default=69)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--torch-reps", type=int, default=3)
    o = ap.parse_args()
    g = torch.Generator(device=DEV).manual_seed(0)
    X = torch.rand(o.rows, o.dim, generator=g, device=DEV)
    res = {"rows": o.rows, "dim": o.dim, "k": o.k, "device": torch.cuda.get_device_name(0)}
    r2 = metrics.knn_radii(X, o.k)
    res["knn_radii_ms"] = timed(lambda: metrics.knn_radii(X, o.k), 5)
    pairs = float(o.rows) * o.rows * o.dim
    res["knn_radii_tpairs_per_s"] = pairs / (res["knn_radii_ms"] * 1e-3) / 1e12
    for m in (16384, 64):
        Q = X[:m]
        res["ball_query_%d_ms" % m] = timed(lambda: metrics.ball_query(Q, X, r2), 5)
        res["nearest_%d_ms" % m] = timed(lambda: metrics.ball_query(Q, X), 5)
    say(json.dumps(res))
    r = r2.sqrt()
    for tag, mode in (("direct", "donot_use_mm_for_euclid_dist"), ("mm", "use_mm_for_euclid_dist")):
        if o.torch_reps <= 0:
            break
        # the direct form runs one workgroup per pair: an eighth of the rows is timed, and the key says so
        sub = None if tag == "mm" else max(o.rows // 8, 1)
        key = "torch_%s_radii_ms" % tag if sub is None else "torch_%s_radii_first_%d_rows_ms" % (tag, sub)
        res[key] = timed(lambda: torch_radii(X, o.k, mode, sub), o.torch_reps)
        say(key, res[key])
        for m in (16384, 64):
            Q = X[:m]
            res["torch_%s_query_%d_ms" % (tag, m)] = timed(lambda: torch_query(Q, X, r, mode), o.torch_reps)
            say(tag, m, res["torch_%s_query_%d_ms" % (tag, m)])
        t = torch_radii(X[:4096], o.k, mode) if o.rows <= 4096 else torch.cat(
            [torch.kthvalue(torch.cdist(X[i:i + 64], X, compute_mode=mode), o.k + 1, dim=1).values ** 2
             for i in range(0, 4096, 64)])
        res["torch_%s_radii_max_rel_diff" % tag] = float(((t - r2[:4096]).abs() / r2[:4096]).max())
        del t
    print(json.dumps(res))


if __name__ == "__main__":
    main()
