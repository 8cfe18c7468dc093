"""Time and peak memory of the sample metrics at n = 8192, d in {2, 16, 128} (profiles/metrics_kernels.log):
Sinkhorn (100 iterations) and MMD through the HIP kernels against a dense float32 torch composition of the same arithmetic on the
same GPU, and the sliced KS distance on the GPU against the reference-style CPU loop (one torch.histogram per projection).
Each timing is the median of REPS calls after a warm-up call, wall clock around a device synchronise."""
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from sde_sampler_lrds_amd import engine as E  # noqa: E402
from sde_sampler_lrds_amd.additions.ks import compute_sliced_ks  # noqa: E402
from tests.test_gpu_metrics import _dense_mmd, _dense_sinkhorn  # noqa: E402  (the dense restatements the tests compare against)

N, REPS = 8192, 5
dev = torch.device("cuda:0")


def measure(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base, ts = torch.cuda.memory_allocated(), []
    for _ in range(REPS):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return out, statistics.median(ts), min(ts), max(ts), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def ks_cpu_loop(s1, s2, projs, n_bins=256):
    """additions/ks.py of the reference: samples copied to the CPU, one torch.histogram per projection."""
    s1, s2 = s1.cpu(), s2.cpu()
    p1, p2 = projs @ s1.T, projs @ s2.T
    lo, hi = p1.min(-1).values, p1.max(-1).values
    cdfs = []
    for p in (p1, p2):
        h = torch.stack([torch.histogram(p[i], bins=n_bins, range=(float(lo[i]), float(hi[i]))).hist for i in range(projs.shape[0])])
        cdfs.append((h / h.sum(-1, keepdim=True)).cumsum(-1))
    return (cdfs[0] - cdfs[1]).abs().max(-1).values.mean()


def main():
    print(f"# n = m = {N}, median [min, max] of {REPS} calls in ms; peak = peak allocated MiB above the inputs")
    for d in (2, 16, 128):
        g = torch.Generator().manual_seed(d)
        x, y = torch.randn(N, d, generator=g).to(dev), (torch.randn(N, d, generator=g) * 1.3 + 0.5).to(dev)
        rows = [("sinkhorn hip (matrix in workspace)", lambda: E.sinkhorn(x, y)["distance"].item()),
                ("sinkhorn hip (costs recomputed)", lambda: E.sinkhorn(x, y, materialise=False)["distance"].item()),
                ("sinkhorn dense torch fp32", lambda: _dense_sinkhorn(x, y)[0]),
                ("mmd hip", lambda: E.mmd_median(x, y)[0].item()),
                ("mmd dense torch fp32", lambda: _dense_mmd(x, y))]
        projs = torch.randn(128, d)
        projs /= torch.linalg.norm(projs, axis=-1)[..., None]
        rows += [("sliced ks torch on the GPU", lambda: compute_sliced_ks(x, y, random_projs=projs).item()),
                 ("sliced ks CPU loop (reference style)", lambda: ks_cpu_loop(x, y, projs).item())]
        for name, fn in rows:
            if d == 128 and "recomputed" in name:
                continue  # O(n m d) per pass: minutes at this size; it is the fallback beyond the matrix cap, timed at d = 2 and 16
            out, med, lo, hi, peak = measure(fn)
            print(f"d={d:<4d} {name:<38s} {med:10.2f} [{lo:.2f}, {hi:.2f}] ms  peak {peak:9.1f} MiB  value {out:.6g}", flush=True)


if __name__ == "__main__":
    main()
