"""Helpers shared by the PAG test files (test_gpu_pag_ops.py, test_gpu_pag.py): error measures, one realistic coefficient row per
first-order step kind, the case list of the step kernels, and a stub VAE for ``log_validation``.  No test lives here."""
import numpy as np
import torch

DDIM, RESSHIFT, DDPM, UNIPC, DPMSOLVERPP = 0, 1, 2, 3, 4


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-12))


def maxrel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def coef_row(kind, a_t=0.37, a_p=0.52):
    """One coefficient row per step kind, as mrisr_sampler_create builds them (rounded to f32: kernel and reference read the same
    numbers)."""
    if kind == DDIM:
        row = [np.sqrt(a_p / a_t), np.sqrt(1 - a_p) - np.sqrt(a_p * (1 - a_t) / a_t)]
    elif kind == RESSHIFT:
        row = [np.sqrt(a_t), np.sqrt(1 - a_t), np.sqrt(a_p), np.sqrt((1 - a_p) / (1 - a_t) * (1 - a_t / a_p))]
    else:
        al = a_t / a_p
        row = [1 / np.sqrt(a_t), np.sqrt(1 - a_t) / np.sqrt(a_t), np.sqrt(a_p) * (1 - al) / (1 - a_t),
               np.sqrt(al) * (1 - a_p) / (1 - a_t), np.sqrt((1 - a_p) / (1 - a_t) * (1 - al))]
    return [float(np.float32(r)) for r in row]


def kernel_cases():
    """(kind, with noise, clip) of the first-order step kinds."""
    for kind in (DDIM, RESSHIFT, DDPM):
        for with_noise in ((False,) if kind == DDIM else (False, True)):
            for clip in ((0.0, 1.0) if kind == DDPM else (0.0,)):
                yield kind, with_noise, clip


class StubVAE:
    """8x average-pool 'encoder' and nearest 'decoder': enough for ``log_validation`` to run end to end."""

    class config:
        scaling_factor = 0.18215

    def encode(self, x):
        z = torch.nn.functional.avg_pool2d(x[:, :1], 8).repeat(1, 4, 1, 1)
        return type("E", (), {"latent_dist": type("D", (), {"sample": staticmethod(lambda: z)})})

    def decode(self, z):
        return type("O", (), {"sample": torch.nn.functional.interpolate(z.mean(1, keepdim=True), scale_factor=8.0, mode="nearest")})
