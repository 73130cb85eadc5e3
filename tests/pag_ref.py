"""Reference for perturbed-attention guidance (PAG; Ahn et al. 2024), shared by test_pag_cpu.py (which checks THIS file on the CPU)
and test_gpu_pag.py (which checks the device path against it).  No new oracle code:

* ``perturbed_attention(prefixes)`` swaps ``oracle.unet.attention`` for a wrapper while it is active.  For the self-attention
  (names ending ``.attn1``) of every transformer block under one of ``prefixes`` the wrapper returns
  ``linear(to_out.0, linear(to_v, x))`` - the attention map is the identity, every token's output is its own value vector, the
  heads concatenated as usual, the LoRA terms of both projections kept - on the perturbed rows, and calls the original otherwise.
* ``PagUNet`` mirrors ``GuidedUNet`` of guidance_ref.py: it evaluates the wrapped network plainly (eps_c, and eps_u with
  classifier-free guidance) and under ``perturbed_attention`` (eps_p) and combines in float64:

      PAG alone:     e = eps_c + s (eps_c - eps_p)
      PAG with CFG:  e = eps_u + g (eps_c - eps_u) + s (eps_c - eps_p)
      phi > 0:       e = e (phi std(eps_c) / std(e) + (1 - phi))       torch.std over (C, h, w) of every sample, unbiased

  ControlNet residuals and adapter features are never perturbed: the perturbed call receives those of its conditional twin."""
import contextlib


def block_names(cfg):
    """The transformer blocks of the oracle's UNet in forward order (the names ``oracle.unet.unet_forward`` walks)."""
    n = cfg.num_levels
    names = [f"down_blocks.{i}.attentions.{j}" for i in range(n) if cfg.attn_levels[i] for j in range(cfg.layers_per_block)]
    names.append("mid_block.attentions.0")
    names += [f"up_blocks.{i}.attentions.{j}" for i in range(n) if cfg.attn_levels[n - 1 - i] for j in range(cfg.layers_per_block + 1)]
    return names


def _selects(prefix, name):
    """``prefix`` selects ``name`` when it matches at a component boundary; "mid" stands for "mid_block"."""
    parts = prefix.split(".")
    if parts[0] == "mid":
        parts[0] = "mid_block"
    return name.split(".")[:len(parts)] == parts


def mask_of(prefixes, names):
    m = 0
    for p in prefixes:
        hit = [i for i, n in enumerate(names) if _selects(p, n)]
        assert hit, (p, names)
        for i in hit:
            m |= 1 << i
    return m


@contextlib.contextmanager
def perturbed_attention(prefixes, rows=None):
    """While active, ``attn1`` of the selected blocks is the identity-attention form on ``rows`` (a slice / index of the batch; None: all)."""
    from oracle import unet as ou
    orig = ou.attention
    prefixes = tuple(prefixes)

    def attention(p, name, x, ctx, heads, lora_scale):
        if not (name.endswith(".attn1") and any(_selects(q, name) for q in prefixes)):
            return orig(p, name, x, ctx, heads, lora_scale)
        pert = ou.linear(p, name + ".to_out.0", ou.linear(p, name + ".to_v", x, lora_scale), lora_scale)
        if rows is None:
            return pert
        out = orig(p, name, x, ctx, heads, lora_scale).clone()
        out[rows] = pert[rows]
        return out

    ou.attention = attention
    try:
        yield
    finally:
        ou.attention = orig


def pag_eps(eps_p, eps_u, eps_c, g, s, phi):
    """The combined prediction in float64; ``eps_u`` None: PAG alone."""
    eps_p, eps_c = eps_p.double(), eps_c.double()
    e = eps_c if eps_u is None else eps_u.double() + g * (eps_c - eps_u.double())
    e = e + s * (eps_c - eps_p)
    if phi > 0:
        e = e * (phi * eps_c.std(dim=(1, 2, 3), keepdim=True) / e.std(dim=(1, 2, 3), keepdim=True) + (1 - phi))
    return e


class _Out:
    def __init__(self, sample):
        self.sample = sample


class CtxControlNet:
    """The ControlNet with a fixed context (the loop's own ``encoder_hidden_states`` is ignored), for PAG alone: one set of residuals
    that the conditional and the perturbed call share."""

    def __init__(self, controlnet, ctx):
        self.controlnet, self.ctx = controlnet, ctx

    def __call__(self, sample, timestep, encoder_hidden_states=None, controlnet_cond=None, return_dict=False):
        return self.controlnet(sample, timestep, encoder_hidden_states=self.ctx, controlnet_cond=controlnet_cond, return_dict=False)


class PagUNet:
    """``unet`` evaluated with ``ctx_c`` plainly and perturbed (and with ``ctx_u`` plainly when given); ``.sample`` is the combined
    prediction in the sample's dtype.  ``last`` keeps (eps_p, eps_u or None, eps_c, e float64) of the latest call.  ControlNet
    residuals: one (down, mid) as ``CtxControlNet`` returns, or ((down_u, down_c), (mid_u, mid_c)) of ``GuidedControlNet``."""

    def __init__(self, unet, ctx_c, pag_scale, layers, ctx_u=None, guidance_scale=1.0, guidance_rescale=0.0):
        self.unet, self.ctx_c, self.ctx_u = unet, ctx_c, ctx_u
        self.s, self.g, self.phi = float(pag_scale), float(guidance_scale), float(guidance_rescale)
        self.layers = tuple(layers)
        self.last = None

    def _call(self, sample, timestep, ctx, down, mid, intra):
        kw = {}
        if down is not None:
            kw = dict(down_block_additional_residuals=down, mid_block_additional_residual=mid)
        if intra is not None:  # the UNet adds into its skip list in place: a fresh copy per call
            kw["down_intrablock_additional_residuals"] = [f.clone() for f in intra]
        return self.unet(sample, timestep, encoder_hidden_states=ctx, **kw).sample

    def __call__(self, sample, timestep, encoder_hidden_states=None, down_block_additional_residuals=None,
                 mid_block_additional_residual=None, down_intrablock_additional_residuals=None):
        down, mid, intra = down_block_additional_residuals, mid_block_additional_residual, down_intrablock_additional_residuals
        pair = down is not None and isinstance(down, tuple) and len(down) == 2 and isinstance(down[0], (list, tuple))
        d_u, m_u = (down[0], mid[0]) if pair else (down, mid)
        d_c, m_c = (down[1], mid[1]) if pair else (down, mid)
        eps_c = self._call(sample, timestep, self.ctx_c, d_c, m_c, intra)
        eps_u = self._call(sample, timestep, self.ctx_u, d_u, m_u, intra) if self.ctx_u is not None else None
        if self.s == 0.0 and not self.layers:
            eps_p = eps_c
        else:
            with perturbed_attention(self.layers):
                eps_p = self._call(sample, timestep, self.ctx_c, d_c, m_c, intra)
        e = pag_eps(eps_p, eps_u, eps_c, self.g, self.s, self.phi)
        self.last = (eps_p, eps_u, eps_c, e)
        return _Out(e.to(sample.dtype))
