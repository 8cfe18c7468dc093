"""Test helper shared by the GPU sampler tests (tests/test_gpu_rwmh.py, tests/test_make_model_gpu.py)."""
import torch


class CpuGenerator:
    """Draw every random number of the samplers from torch's CPU generator (the one the fixtures were generated with) and move it to
    the chains' device: same seed, same consumption order -> the reference's random numbers, on GPU tensors."""

    def __enter__(self):
        self.saved = {n: getattr(torch, n) for n in ("randn", "rand", "randn_like", "rand_like", "multinomial")}
        s = self.saved

        def shaped(fn):
            def wrap(*size, device=None, dtype=None, generator=None, **kw):
                return fn(*size, dtype=dtype, **kw).to(device or "cpu")
            return wrap
        torch.randn, torch.rand = shaped(s["randn"]), shaped(s["rand"])
        torch.randn_like = lambda t, **kw: s["randn"](t.shape, dtype=t.dtype).to(t.device)
        torch.rand_like = lambda t, **kw: s["rand"](t.shape, dtype=t.dtype).to(t.device)
        torch.multinomial = lambda w, n, replacement=False, **kw: s["multinomial"](w.cpu(), n, replacement=replacement).to(w.device)
        return self

    def __exit__(self, *exc):
        for n, f in self.saved.items():
            setattr(torch, n, f)
