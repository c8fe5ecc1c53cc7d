"""pg_affine_rows -- the eval-mode VAE encoder as one affine map of the rows of the two normalised matrices (csrc/encode.hip) --
and ``VAENET.encode`` through it: the kernel against float64, the encode against the layers evaluated in float64 on the CPU,
batching, the fallbacks to the layered path, the refusals, and one pass through the checked build; and pg_affine_fold, the fold of
one layer in one kernel, against the fold as tensor operations."""
import copy
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from pangaea_amd import _lib
from pangaea_amd.data import Data
from pangaea_amd.models.VAENET import VAENET, VaritionalAutoEncoder

from .conftest import ROOT
from .test_encode_fold import NETS, randomise_batchnorm
from .test_vae_data import _g5

pytestmark = pytest.mark.gpu

# rows around a wavefront and a row tile, a K that is no multiple of the K-tile with the tile's edge inside abd and inside tnf,
# the widest output, no rows at all
SHAPES = [(1, 1, 1, 1), (63, 400, 136, 32), (64, 400, 136, 32), (65, 400, 136, 32), (257, 63, 65, 32), (1000, 400, 136, 32),
          (130, 512, 32, 64), (0, 400, 136, 32)]
GUARD = 3                     # rows in front of and behind the output that the kernel must leave alone
SENTINEL = -12345.0


def _ordered(a: np.ndarray) -> np.ndarray:
    """float32 -> integers in which neighbouring floats differ by one"""
    i = a.view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def _ulps(a: np.ndarray, b: np.ndarray) -> int:
    return int(np.abs(_ordered(a) - _ordered(b)).max()) if a.size else 0


def _affine(abd, tnf, w, b, n_out):
    """pg_affine_rows on device tensors; the output lies between guard rows, which are checked"""
    L = _lib.load()
    n = abd.shape[0]
    buf = torch.full((n + 2 * GUARD, n_out), SENTINEL, dtype=torch.float32, device="cuda:0")
    out = buf[GUARD:GUARD + n]
    _lib.check(L.pg_affine_rows(abd.data_ptr(), abd.shape[1], tnf.data_ptr(), tnf.shape[1], n, w.data_ptr(), b.data_ptr(), n_out,
                                out.data_ptr(), None))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    assert (host[:GUARD] == SENTINEL).all() and (host[GUARD + n:] == SENTINEL).all(), "a store outside the output rows"
    return host[GUARD:GUARD + n]


@pytest.mark.parametrize("n_rows,n_abd,n_tnf,n_out", SHAPES, ids=lambda v: str(v))
def test_kernel_against_float64(n_rows, n_abd, n_tnf, n_out):
    rs = np.random.RandomState(n_rows + n_abd + n_out)
    abd = rs.rand(n_rows, n_abd).astype(np.float32)
    tnf = (rs.rand(n_rows, n_tnf) * 4 - 1).astype(np.float32)
    w, b = rs.randn(n_abd + n_tnf, n_out), rs.randn(n_out)
    want = (np.concatenate([abd, tnf], axis=1).astype(np.float64) @ w + b).astype(np.float32)
    dev = [torch.from_numpy(a).cuda() for a in (abd, tnf, w, b)]
    got = _affine(*dev, n_out)
    assert got.shape == want.shape
    worst = _ulps(got, want)
    print(f"pg_affine_rows {(n_rows, n_abd, n_tnf, n_out)}: worst difference to float64 numpy narrowed to float32 = {worst} ulp")
    assert worst <= 2


def test_rows_do_not_depend_on_their_batch():
    """one chain of sums per output, whatever the grid: a row gives the same bits alone, at the end of a tile and in the middle"""
    rs = np.random.RandomState(9)
    abd, tnf = rs.rand(300, 400).astype(np.float32), rs.rand(300, 136).astype(np.float32)
    w, b = torch.from_numpy(rs.randn(536, 32)).cuda(), torch.from_numpy(rs.randn(32)).cuda()
    A, T = torch.from_numpy(abd).cuda(), torch.from_numpy(tnf).cuda()
    whole = _affine(A, T, w, b, 32)
    for lo, hi in ((0, 1), (127, 129), (171, 300), (299, 300)):
        assert np.array_equal(_affine(A[lo:hi], T[lo:hi], w, b, 32), whole[lo:hi]), (lo, hi)
    # rows whose length is no multiple of 4 are read one float at a time: same sums, same bits
    A0 = A.clone()
    A0[:, 0] = 0                                                      # (fma(0, w, b) = b: the chain of the 399 columns)
    assert np.array_equal(_affine(A[:, 1:].contiguous(), T, w[1:], b, 32), _affine(A0, T, w, b, 32))


def _fold_nets():
    for kind, kw in NETS.items():
        yield kind, (400, 136), kw, False
    yield "odd_sizes", (399, 135), {"hidden_sizes": (61, 7), "latent_size": 33}, False       # nothing a multiple of 4, a latent beyond 32
    yield "plain_layers", (400, 136), {"hidden_sizes": (64, 48)}, True                       # BatchNorm1d without gamma / beta, Linear without bias


@pytest.mark.parametrize("kind,sizes,kw,plain", list(_fold_nets()), ids=lambda v: v if isinstance(v, str) else "")
def test_fold_on_the_gpu_is_the_fold_on_the_cpu(kind, sizes, kw, plain, monkeypatch):
    """pg_affine_fold (one kernel per Linear + BatchNorm1d) against the same fold as float64 tensor operations on the CPU, which
    tests/test_encode_fold.py holds against the layers themselves"""
    torch.manual_seed(17)
    net = VaritionalAutoEncoder(*sizes, **kw)
    if plain:
        net.encoder[1] = torch.nn.BatchNorm1d(64, affine=False)
        net.encoder[4] = torch.nn.Linear(64, 48, bias=False)
    randomise_batchnorm(net, 4)
    net.eval()
    want_w, want_b = net.affine_encoder()
    L = _lib.load()
    real, calls = L.pg_affine_fold, []
    monkeypatch.setattr(L, "pg_affine_fold", lambda *a: calls.append(a[7:9]) or real(*a))
    got_w, got_b = net.cuda().affine_encoder()
    assert len(calls) == len(kw.get("hidden_sizes", (512, 512))) + 1, calls        # every layer went through the kernel
    assert got_w.is_cuda and got_w.dtype == torch.float64 and got_w.is_contiguous() and got_w.shape == want_w.shape
    for name, got, want in (("W_eff", got_w, want_w), ("b_eff", got_b, want_b)):
        err = float((got.cpu() - want).abs().max() / want.abs().max())
        print(f"{kind}: {name} of pg_affine_fold against the tensor-operation fold, max |diff| / max = {err:.3e}")
        assert err <= 1e-12


def test_fold_refusals():
    L = _lib.load()
    w = torch.zeros((8, 16), dtype=torch.float32, device="cuda:0")
    v = torch.zeros(8, dtype=torch.float32, device="cuda:0")
    a = torch.zeros((8, 4), dtype=torch.float64, device="cuda:0")
    o = torch.zeros((16, 4), dtype=torch.float64, device="cuda:0")
    p = lambda t: t.data_ptr()

    def refused(name, *args):
        assert L.pg_affine_fold(*args) == -1
        msg = L.pg_last_error().decode()
        assert "pg_affine_fold" in msg and name in msg, msg
    good = [p(w), p(v), p(v), p(v), p(v), p(v), 1e-5, 16, 8, p(a), p(a), 4, p(o), p(o), None]
    assert L.pg_affine_fold(*good) == 0
    for i, value, name in ((0, None, "weight"), (12, None, "a_out"), (13, None, "c_out"), (3, None, "bn_var"), (7, 0, "n_in"), (8, -1, "n_mid"),
                           (11, 65, "n_out"), (9, None, "a is null")):
        args = list(good)
        args[i] = value
        refused(name, *args)
    args = list(good)
    args[2] = args[3] = None                                          # gamma without statistics
    refused("bn_gamma", *args)
    torch.cuda.synchronize()


def _net(randomised: bool):
    _, state = _g5("vae_g5b_512.npz")
    vae = VAENET(400, 136, 32, 30, 1, True, 1, 0.005, 0.2, 0.1, 0.015, 0.0001)
    vae.network.load_state_dict({k: torch.from_numpy(v) for k, v in state.items()})
    if randomised:
        randomise_batchnorm(vae.network, 21)
    vae.network.eval()
    return vae


def _data(n: int, seed: int = 3) -> Data:
    rs = np.random.RandomState(seed)
    abd = torch.from_numpy(rs.poisson(2.0, (n, 400)).astype(np.int32)).cuda()
    tnf = torch.from_numpy(rs.poisson(30.0, (n, 136)).astype(np.int32)).cuda()
    return Data(np.arange(n), abd, tnf)


@pytest.mark.parametrize("randomised", [False, True], ids=["golden_state", "random_batchnorm"])
def test_encode_against_the_layers_in_float64(randomised, monkeypatch):
    """the reference value: the layered module in float64 on the CPU, fed with the float32 inputs cast up"""
    vae = _net(randomised)
    g, _ = _g5("vae_g5b_512.npz")
    ref_net = copy.deepcopy(vae.network).double().cpu()
    golden = SimpleNamespace(abd_dev=torch.from_numpy(g["abd"]).cuda(), tnf_dev=torch.from_numpy(g["tnf"]).cuda())    # (normalised already)
    for what, d in (("golden rows", golden), ("1000 rows", _data(1000))):
        with torch.no_grad():
            ref = ref_net.emebdding(d.abd_dev.cpu().double(), d.tnf_dev.cpu().double()).numpy()
        monkeypatch.setenv("PG_ENCODE_FUSED", "1")
        fused = vae.encode(d).cpu().numpy().astype(np.float64)
        monkeypatch.setenv("PG_ENCODE_FUSED", "0")
        layered = vae.encode(d).cpu().numpy().astype(np.float64)
        scale = np.abs(ref).max()
        err_layered, err_fused = np.abs(layered - ref).max(), np.abs(fused - ref).max()
        print(f"encode, {'random BatchNorm' if randomised else 'golden state'}, {what}: max |mu| = {scale:.4g}, "
              f"err_layered = {err_layered:.3e} ({err_layered / scale:.2e} of max), err_fused = {err_fused:.3e} ({err_fused / scale:.2e} of max)")
        assert err_fused <= max(2 * err_layered, 1e-6 * scale)
        assert err_fused <= 1e-5 * scale
        if d is golden and not randomised:
            assert np.abs(fused - g["mu"]).max() <= 1e-5 * np.abs(g["mu"]).max()        # the reference's own vectors


def test_encode_in_slices_is_bit_identical(monkeypatch):
    monkeypatch.setenv("PG_ENCODE_FUSED", "1")
    vae, d = _net(True), _data(257)
    calls = _count_calls(monkeypatch)
    whole = vae.encode(d)
    assert calls == [257]
    assert torch.equal(vae.encode(d, batch_rows=100), whole)
    assert calls == [257, 100, 100, 57]


def _count_calls(monkeypatch) -> list:
    """wraps pg_affine_rows of the loaded library; the list receives n_rows of every call"""
    L = _lib.load()
    real, calls = L.pg_affine_rows, []

    def counting(*args):
        calls.append(int(args[4]))
        return real(*args)
    monkeypatch.setattr(L, "pg_affine_rows", counting)
    return calls


def test_switch_runs_the_layers(monkeypatch):
    vae, d = _net(True), _data(257)
    calls = _count_calls(monkeypatch)
    with torch.no_grad():
        layered = vae.network.emebdding(d.abd_dev, d.tnf_dev)
    monkeypatch.setenv("PG_ENCODE_FUSED", "0")
    assert torch.equal(vae.encode(d), layered) and calls == []
    monkeypatch.setenv("PG_ENCODE_FUSED", "1")
    fused = vae.encode(d)
    assert calls == [257]
    assert float((fused - layered).abs().max()) <= 2e-5 * float(layered.abs().max())      # (each within 1e-5 of the float64 value)


def test_a_real_activation_runs_the_layers(monkeypatch):
    monkeypatch.delenv("PG_ENCODE_FUSED", raising=False)
    vae, d = _net(True), _data(257)
    vae.network.encoder[2] = torch.nn.LeakyReLU(0.01)
    calls = _count_calls(monkeypatch)
    got = vae.encode(d)
    with torch.no_grad():
        assert torch.equal(got, vae.network.emebdding(d.abd_dev, d.tnf_dev))
    assert calls == []
    # inputs that are not contiguous float32 matrices take the layers too
    vae = _net(True)
    strided = SimpleNamespace(abd_dev=torch.rand(50, 800, device="cuda:0")[:, ::2], tnf_dev=torch.rand(50, 136, device="cuda:0"))
    got = vae.encode(strided)
    with torch.no_grad():
        assert torch.equal(got, vae.network.emebdding(strided.abd_dev, strided.tnf_dev))
    assert calls == []


def test_refusals():
    L = _lib.load()
    x = torch.zeros((4, 8), dtype=torch.float32, device="cuda:0")
    w = torch.zeros((16, 65), dtype=torch.float64, device="cuda:0")
    o = torch.zeros((4, 65), dtype=torch.float32, device="cuda:0")
    p = lambda t: t.data_ptr()

    def refused(name, *args):
        assert L.pg_affine_rows(*args) == -1                       # PG_EINVAL
        msg = L.pg_last_error().decode()
        assert "pg_affine_rows" in msg and name in msg, msg
    refused("n_out", p(x), 8, p(x), 8, 4, p(w), p(w), 65, p(o), None)
    refused("n_out", p(x), 8, p(x), 8, 4, p(w), p(w), 0, p(o), None)
    refused("n_rows", p(x), 8, p(x), 8, -1, p(w), p(w), 32, p(o), None)
    refused("n_abd + n_tnf", p(x), 0, p(x), 0, 4, p(w), p(w), 32, p(o), None)
    refused("n_abd", p(x), -8, p(x), 8, 4, p(w), p(w), 32, p(o), None)
    for i, name in ((0, "abd"), (2, "tnf"), (5, "w"), (6, "b"), (8, "out")):
        args = [p(x), 8, p(x), 8, 4, p(w), p(w), 32, p(o), None]
        args[i] = None
        refused(name + " is null", *args)
    assert L.pg_affine_rows(None, 8, None, 8, 0, None, None, 32, None, None) == 0       # no rows: nothing to do, nothing looked at
    assert L.pg_affine_rows(None, 0, p(x), 8, 4, p(w), p(w), 32, p(o), None) == 0       # a matrix without columns may be null
    torch.cuda.synchronize()


def test_through_the_checked_build():
    """new kernel code runs through the library built with -DPG_CHECKED first: the other tests of this
    file in a process of their own with PANGAEA_LIB=checked"""
    env = dict(os.environ, PANGAEA_LIB="checked")
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", os.path.join(ROOT, "tests", "test_encode_affine_gpu.py"),
                        "-k", "not through_the_checked_build"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "no tests ran" not in r.stdout
