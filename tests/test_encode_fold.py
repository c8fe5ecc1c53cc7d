"""``VaritionalAutoEncoder.affine_encoder``: the eval-mode encoder (Linear, BatchNorm1d on its running statistics, the identity
``LeakyReLU(True)``, Dropout, l_mu) folded into one float64 affine map -- against the module's own layers in float64, and the
cases in which the stack is NOT affine and the fold must say so.  CPU only."""
import copy

import pytest
import torch
import torch.nn as nn

from pangaea_amd.models.VAENET import VaritionalAutoEncoder

NETS = {"default": {}, "two_small": {"hidden_sizes": (64, 48)}, "one_layer": {"hidden_sizes": (96,)}}


def randomise_batchnorm(net: nn.Module, seed: int) -> None:
    """running statistics and gamma / beta that are nowhere near 0 / 1: the defaults would hide a wrong fold"""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm1d):
                n = m.num_features
                if m.running_mean is not None:
                    m.running_mean.copy_(torch.randn(n, generator=g))
                    m.running_var.copy_(0.3 + 2.7 * torch.rand(n, generator=g))           # [0.3, 3]
                if m.weight is not None:
                    m.weight.copy_((0.5 + torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1))
                    m.bias.copy_(torch.randn(n, generator=g))


def make_net(kind: str, seed: int = 11) -> VaritionalAutoEncoder:
    torch.manual_seed(seed)
    net = VaritionalAutoEncoder(400, 136, **NETS[kind])
    randomise_batchnorm(net, seed + 1)
    return net.eval()


@pytest.mark.parametrize("kind", list(NETS))
def test_fold_equals_the_layers_in_float64(kind):
    net = make_net(kind)
    fold = net.affine_encoder()
    assert fold is not None
    w, b = fold
    assert w.dtype == torch.float64 and b.dtype == torch.float64 and w.is_contiguous()
    assert tuple(w.shape) == (536, 32) and tuple(b.shape) == (32,)
    g = torch.Generator().manual_seed(5)
    abd, tnf = torch.rand(97, 400, generator=g), torch.rand(97, 136, generator=g)
    abd, tnf = abd / abd.sum(1, keepdim=True), tnf / tnf.sum(1, keepdim=True)          # L1-normalised rows, as Data leaves them
    with torch.no_grad():
        want = copy.deepcopy(net).double().emebdding(abd.double(), tnf.double())
    got = torch.cat((abd, tnf), 1).double() @ w + b
    err = float((got - want).abs().max() / want.abs().max())
    print(f"{kind}: fold against the float64 layers, max |diff| / max |mu| = {err:.3e}")
    assert err <= 1e-12
    assert all(p.dtype == torch.float32 for p in net.parameters())                     # the fold left the module alone


def test_no_fold_in_training_mode():
    net = make_net("default")
    net.train()
    assert net.affine_encoder() is None
    net.eval()
    assert net.affine_encoder() is not None
    net.encoder[3].train()                                                             # one active Dropout is enough
    assert net.affine_encoder() is None


def test_no_fold_with_a_real_leaky_relu():
    net = make_net("default")
    net.encoder[2] = nn.LeakyReLU(0.01)
    assert net.eval().affine_encoder() is None
    net.encoder[2] = nn.LeakyReLU(True)
    assert net.affine_encoder() is not None
    net.encoder[6] = nn.ReLU()                                                         # nor with any module the fold does not know
    assert net.affine_encoder() is None


def test_no_fold_without_running_statistics():
    net = make_net("default")
    net.encoder[1] = nn.BatchNorm1d(512, track_running_stats=False)
    assert net.eval().affine_encoder() is None


def test_fold_of_plain_variants():
    """a BatchNorm1d without gamma / beta and a Linear without bias fold too"""
    net = make_net("two_small")
    net.encoder[1] = nn.BatchNorm1d(64, affine=False)
    net.encoder[4] = nn.Linear(64, 48, bias=False)
    randomise_batchnorm(net, 3)
    net.eval()
    w, b = net.affine_encoder()
    x = torch.rand(9, 536, generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = copy.deepcopy(net).double().emebdding(x[:, :400].double(), x[:, 400:].double())
    assert float((x.double() @ w + b - want).abs().max() / want.abs().max()) <= 1e-12
