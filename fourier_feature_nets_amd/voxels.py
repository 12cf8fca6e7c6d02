"""Dense voxel radiance field ("voxels" checkpoints of the reference, voxels_model.py:9-56): a
(1,4,S,S,S) volume of raw [r,g,b,sigma] logits over the cube [-scale, scale]^3, looked up
trilinearly by the HIP kernel K10 (``csrc/occupancy.hip``).  State-dict keys (``voxels``,
``bias``), ``params`` and the ``save`` format are the reference's, so checkpoints go both ways.

It is the opacity model of the focus sampler, and it is trained like the reference's
train_voxels.py: ``Raycaster.fit`` runs its steps through ``TrainEngine`` with ``VoxelProgram``
(K10 forward, K10b backward in ``csrc/voxels.hip``, the shared clip+Adam kernel) over one flat
[volume | bias] buffer.  ``Voxels.forward`` itself stays inference-only: under autograd it raises.
``Voxels`` deliberately has no ``program`` attribute -- the focus sampler and the fused render
choose the fused-MLP kernels by it."""

import torch
import torch.nn as nn

from . import ops


class Voxels(nn.Module):
    use_view = False

    def __init__(self, side: int, scale: float):
        super().__init__()
        self.params = dict(side=side, scale=scale)
        self.scale = scale
        self.voxels = nn.Parameter(torch.zeros((1, 4, side, side, side), dtype=torch.float32))
        # the reference starts from (almost) black and sigma logit -2
        start = torch.full((4,), float(torch.logit(torch.tensor(1e-5))), dtype=torch.float32)
        start[3] = -2.0
        self.bias = nn.Parameter(start.reshape(1, 4))

    def forward(self, positions: torch.Tensor) -> torch.Tensor:
        """(N,3) world positions -> (N,4) raw logits."""
        if torch.is_grad_enabled() and (self.voxels.requires_grad or self.bias.requires_grad):
            raise NotImplementedError("Voxels is an inference-only opacity model here (wrap the "
                                      "call in torch.no_grad()); training the volume is outside "
                                      "the HIP hot path")
        side = self.voxels.shape[-1]
        out = ops.voxels_forward(self.voxels.detach().reshape(4, side, side, side).contiguous(),
                                 self.bias.detach().reshape(4).contiguous(),
                                 positions.reshape(-1, 3).contiguous(), side, float(self.scale))
        return out

    def _dense_params(self):
        """The trained parameters in the reference's order (its ``Adam(model.parameters())``):
        the flat buffer, the Adam moments and ``state_dict()`` line up with it."""
        return [self.voxels, self.bias]

    def invalidate_packed(self):
        """(The kernels read the parameters directly: nothing is cached.)"""

    def save(self, path: str):
        blob = self.state_dict()
        blob["type"] = "voxels"
        blob["params"] = self.params
        torch.save(blob, path)


class VoxelProgram:
    """The kernel surface ``TrainEngine`` drives for a ``Voxels`` model -- the subset of
    ``MlpProgram`` a training step uses: K10 forward, K10b backward into the flat gradient
    buffer ``[volume | bias]``.  One arithmetic: ``precision`` is accepted and ignored."""

    def __init__(self, model: Voxels):
        self.model = model
        self.side = int(model.voxels.shape[-1])
        self.scale = float(model.scale)
        self.num_grad_floats = 4 * self.side ** 3 + 4

    @staticmethod
    def plan_blocks(n: int) -> int:
        return (n + 31) // 32

    def saved_floats(self, n: int) -> int:
        """Floats of the backward's workspace for ``n`` samples (the forward saves nothing)."""
        return (ops.voxels_backward_workspace_bytes(n, self.side) + 3) // 4

    def forward(self, positions: torch.Tensor, views=None, saved=None, precision: str = "f32"):
        """K10: positions (N,3) -> logits (N,4)."""
        side = self.side
        return ops.voxels_forward(self.model.voxels.detach().reshape(4, side, side, side),
                                  self.model.bias.detach().reshape(4), positions.contiguous(),
                                  side, self.scale)

    def backward(self, d_logits: torch.Tensor, positions: torch.Tensor, views, saved: torch.Tensor,
                 grads: torch.Tensor, precision: str = "f32"):
        """K10b: overwrites ``grads`` (num_grad_floats) with [d volume | d bias]."""
        cut = 4 * self.side ** 3
        ops.voxels_backward(positions.contiguous(), d_logits.contiguous(), self.side, self.scale,
                            workspace=saved, d_volume=grads[:cut], d_bias=grads[cut:cut + 4])
