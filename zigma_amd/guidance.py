"""Classifier-free guidance for the samplers.

`Guided(model, cfg_scale, y_null=None)` is a callable with the `(x, t, y)` signature of `model.forward` that evaluates
`ZigMa.forward_guided`: it drops into `Sampler.sample_ode / sample_sde(...)(z, model_fn, y=...)`, `sharded_sampling.sample_sharded` and
`graphs.GraphedForward` unchanged.  The scale lives in a DEVICE tensor that the guided final-layer kernel (zigma_final_layer_cfg_fwd) reads
when it runs: `set_scale()` writes it in place, so a captured graph follows a new scale without a new capture.

The reference has no guided sampling: its `forward_with_cfg` is a stub (model_zigma.py:992-993) and the `cfg_scale` argument of
sample_acc.py:192 is not consumed.
"""
import torch


class Guided:
    def __init__(self, model, cfg_scale, y_null=None):
        """cfg_scale: a float (one scale for every sample) or a (B,) tensor / sequence (one per sample of the batches this is called with).
        y_null: the null condition (forward_guided: the model's null class by default; required for text)."""
        self.model = model
        self.y_null = y_null
        device = next(model.parameters()).device
        self.scale = torch.as_tensor(cfg_scale, dtype=torch.float32).reshape(-1).to(device).clone()

    def set_scale(self, cfg_scale):
        """write the scale(s) into the device tensor in place (same number of values as at construction)"""
        self.scale.copy_(torch.as_tensor(cfg_scale, dtype=torch.float32).reshape(-1))
        return self

    def __call__(self, x, t, y=None):
        return self.model.forward_guided(x, t, y, self.scale, y_null=self.y_null)
