"""Models of fourier_feature_nets_amd that carry the golden weights of tests/golden/models.npz,
shared by the GPU test modules."""

import math

import torch


def load_fourier(g, name, device):
    """A fourier_feature_nets_amd model carrying the golden (or formula-fill) weights ->
    (model on ``device``, (a, b, weights, biases))."""
    import fourier_feature_nets_amd as ffn
    from tests.test_oracle_golden import _fourier_params
    a, b, ws, bs = _fourier_params(g, name)
    channels = [w.shape[0] for w in ws[:-1]]
    model = ffn.FourierFeatureMLP(3, 4, a, b, channels)
    with torch.no_grad():
        for layer, w, bias in zip(model.layers, ws, bs):
            layer.weight.copy_(w)
            layer.bias.copy_(bias)
    return model.to(device), (a, b, ws, bs)


def load_nerf(g, name, skips, inc, device):
    """The golden NeRF ``name`` -> (model on ``device``, its parameters by name)."""
    import fourier_feature_nets_amd as ffn
    from tests.test_oracle_golden import _nerf_params
    p = _nerf_params(g, name)
    n_layers = len([k for k in p if k.startswith("layers.") and k.endswith("weight")])
    ch = p["layers.0.weight"].shape[0]
    fp, fv = p["pos_encoding"].shape[1] // 3, p["view_encoding"].shape[1] // 3
    model = ffn.NeRF(n_layers, ch, math.log2(float(p["pos_encoding"].max())), fp,
                     math.log2(float(p["view_encoding"].max())), fv, skips, inc)
    sd = model.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[name + "/keys"]]
    model.load_state_dict({k: v for k, v in p.items()})
    assert torch.equal(model.pos_encoding.data, p["pos_encoding"])
    return model.to(device), p
