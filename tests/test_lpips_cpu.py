"""CPU-side tests of the LPIPS layer (no GPU): the torch restatement tests/_lpips_ref.py is consistent with itself under `force=`, the
weight loader's key table, the argument errors of consistentnerf_amd.lpips.LPIPS, and the reshaping of io_formats.img2lpips /
run_nerf_view.patch_lpips against the reference's literal lines with a stub model."""
import numpy as np
import pytest
import torch

import _lpips_ref as R


@pytest.fixture(scope="module")
def wts():
    return R.make_weights(0)


def test_restatement_forced_onto_its_own_branches_equals_itself(wts):
    x0, x1 = R.images(2, 16, 21, 3)
    x0, x1 = x0.double().requires_grad_(), x1.double()
    v, taps, taken = R.lpips(x0, x1, wts)
    g, = torch.autograd.grad(v.sum(), x0)
    assert v.shape == (2,) and taps.shape == (5, 2) and len(taken["relu"]) == 13 and len(taken["pool"]) == 4
    vf, tapsf, takenf = R.lpips(x0, x1, wts, force=taken)
    gf, = torch.autograd.grad(vf.sum(), x0)
    assert torch.equal(v, vf) and torch.equal(taps, tapsf) and torch.equal(g, gf)
    assert all(torch.equal(a, b) for a, b in zip(taken["relu"], takenf["relu"]))
    # the seeded weights keep every tap alive: roughly half the units active, no all-zero feature column
    acts, _ = R.trunk((torch.cat([x0.detach(), x1]) - torch.tensor(R.SHIFT).reshape(1, 3, 1, 1).double())
                      / torch.tensor(R.SCALE).reshape(1, 3, 1, 1).double(), wts)
    for l in R.TAPS:
        frac = (acts[l] > 0).double().mean().item()
        assert 0.2 < frac < 0.8, (l, frac)
        assert (acts[l].abs().sum(1) > 0).all()
    # branches_of() reads the same branches back from the activations
    b = R.branches_of(acts)
    assert all(torch.equal(a, c) for a, c in zip(b["relu"], taken["relu"])) and all(torch.equal(a, c) for a, c in zip(b["pool"], taken["pool"]))
    assert float(v.detach().min()) > 0 and torch.allclose(R.lpips(x1, x0.detach(), wts)[0], v.detach(), rtol=1e-12)     # symmetric


def test_loader_key_table_accepts_both_layouts_and_names_bad_keys(wts, tmp_path):
    from consistentnerf_amd import lpips as L
    assert len(L.KEY_TABLE) == 31
    for sd in (R.package_state_dict(wts), R.package_state_dict(wts, lins_prefix=True), R.torchvision_state_dict(wts)):
        st = L.load_state(sd)
        assert len(st) == 33
        for l in range(13):
            assert torch.equal(st[f"conv{l}.weight"], wts["w"][l]) and torch.equal(st[f"conv{l}.bias"], wts["b"][l])
        for k in range(5):
            assert torch.equal(st[f"lin{k}"].reshape(-1), wts["lin"][k])
        assert st["shift"].tolist() == pytest.approx(R.SHIFT) and st["scale"].tolist() == pytest.approx(R.SCALE)
    path = tmp_path / "w.pth"
    torch.save(R.package_state_dict(wts), path)
    assert torch.equal(L.load_state(str(path))["conv12.bias"], wts["b"][12])
    sd = R.package_state_dict(wts)
    del sd["net.slice3.14.weight"]
    with pytest.raises(ValueError, match=r"net\.slice3\.14\.weight"):
        L.load_state(sd)
    sd = R.package_state_dict(wts)
    sd["lin2.model.1.weight"] = sd["lin2.model.1.weight"].reshape(-1)
    with pytest.raises(ValueError, match=r"lin2\.model\.1\.weight has shape"):
        L.load_state(sd)
    sd = R.torchvision_state_dict(wts)
    sd["features.5.bias"] = torch.zeros(64)
    with pytest.raises(ValueError, match=r"features\.5\.bias has shape"):
        L.load_state(sd)
    with pytest.raises(TypeError):
        L.load_state(3)


def test_argument_errors_and_weight_sources(wts, tmp_path, monkeypatch):
    from consistentnerf_amd import lpips as L
    monkeypatch.delenv("CNERF_LPIPS_WEIGHTS", raising=False)
    with pytest.raises(RuntimeError, match="CNERF_LPIPS_WEIGHTS"):
        L.LPIPS(net="vgg")
    sd = R.package_state_dict(wts)
    for kw in (dict(net="alex"), dict(net="squeeze"), dict(spatial=True), dict(lpips=False), dict(version="0.0")):
        with pytest.raises(NotImplementedError):
            L.LPIPS(weights=sd, **kw)
    m = L.LPIPS(net="vgg", weights=sd)
    assert isinstance(m, torch.nn.Module) and not m.training and len(list(m.parameters())) == 0 and len(list(m.buffers())) == 33
    assert set(m.state_dict()) == {n.replace(".", "_") for n in L.KEY_TABLE} | {"shift", "scale"}
    m2 = m.to(torch.float32)                                            # .to() works on the buffers
    assert m2 is m
    x = torch.zeros(1, 3, 16, 16)
    with pytest.raises(TypeError):                                      # CPU tensors
        m(x, x)
    with pytest.raises(TypeError):
        m(x.double(), x.double())
    with pytest.raises(TypeError):
        m(np.zeros((1, 3, 16, 16), np.float32), x)
    # the environment variable serves V:40's bare call
    path = tmp_path / "lpips_vgg.pth"
    torch.save(R.torchvision_state_dict(wts), path)
    monkeypatch.setenv("CNERF_LPIPS_WEIGHTS", str(path))
    m3 = L.LPIPS(net="vgg")
    assert torch.equal(m3.conv7_weight, wts["w"][7]) and torch.equal(m3.lin4.reshape(-1), wts["lin"][4])


def test_shape_errors_are_value_errors(wts, monkeypatch):
    """C != 3 or a side < 16: ValueError (checked after the device / dtype rule, so exercised here on a stand-in for a CUDA tensor)."""
    from consistentnerf_amd import lpips as L

    class T(torch.Tensor):
        is_cuda = True
    mk = lambda *s: torch.zeros(*s).as_subclass(T)  # noqa: E731
    for shape in ((1, 1, 16, 16), (1, 4, 32, 32), (1, 3, 15, 16), (2, 3, 16, 8), (3, 16, 16)):
        with pytest.raises(ValueError):
            L.LPIPS._check(mk(*shape), mk(*shape))
    with pytest.raises(ValueError):
        L.LPIPS._check(mk(1, 3, 16, 16), mk(2, 3, 16, 16))
    L.LPIPS._check(mk(1, 3, 16, 16), mk(1, 3, 16, 16))


class _Stub(torch.nn.Module):
    """A stand-in model: records its inputs, returns a differentiable [N, 1, 1, 1] value."""

    def forward(self, a, b):
        self.seen = (a.detach().clone(), b.detach().clone())
        return ((a - b) ** 2).mean((1, 2, 3)).reshape(-1, 1, 1, 1) + a.mean((1, 2, 3)).reshape(-1, 1, 1, 1)


def test_img2lpips_follows_the_reference_lines():
    from consistentnerf_amd import io_formats as F
    rs = np.random.RandomState(0)
    rgbs, label = rs.uniform(size=(2, 20, 24, 3)).astype(np.float32), rs.uniform(size=(2, 20, 24, 3)).astype(np.float32)
    depth_mask = rs.uniform(size=(2, 20, 24)) > 0.4
    fn = _Stub()
    got = F.img2lpips(rgbs, label, fn)
    # V:2055-2059
    gt, pred = torch.Tensor(label), torch.Tensor(rgbs)
    gt, pred = (gt - 0.5) * 2., (pred - 0.5) * 2.
    gt, pred = gt.permute([0, 3, 1, 2]), pred.permute([0, 3, 1, 2])
    ref = _Stub()
    want = ref(gt, pred).mean()
    assert got.dim() == 0 and torch.equal(got, want) and torch.equal(fn.seen[0], gt) and torch.equal(fn.seen[1], pred)
    assert fn.seen[0].is_contiguous() and fn.seen[0].shape == (2, 3, 20, 24)
    # V:2072-2076
    got = F.img2lpips(torch.from_numpy(rgbs), torch.from_numpy(label), fn, mask=depth_mask)
    mask = np.array([depth_mask, depth_mask, depth_mask]).transpose(1, 0, 2, 3)
    gtm = gt * mask + (1 - mask)
    predm = pred * mask + (1 - mask)
    want = ref(gtm.float(), predm.float()).mean()
    assert torch.equal(got, want) and torch.equal(fn.seen[0], gtm.float()) and torch.equal(fn.seen[1], predm.float())


def test_patch_lpips_follows_the_reference_lines():
    from consistentnerf_amd.run_nerf_view import patch_lpips
    g = torch.Generator().manual_seed(2)
    rgb = torch.rand(5 * 256 + 77, 3, generator=g).requires_grad_()
    target_s = torch.rand(5 * 256 + 77, 3, generator=g)
    fn = _Stub()
    got = patch_lpips(rgb, target_s, fn)
    assert fn.seen[0].shape == (4, 3, 16, 16) and fn.seen[0].is_contiguous()          # ONE batched call
    d_got, = torch.autograd.grad(got[0], rgb)
    # V:1699-1706 + V:1721
    ref = _Stub()
    lpips_fine = 0
    for i_patch in range(4):
        img_pred = rgb[i_patch * 16 * 16: (i_patch + 1) * 16 * 16].reshape(1, 16, 16, 3)
        img_gt = target_s[i_patch * 16 * 16: (i_patch + 1) * 16 * 16].reshape(1, 16, 16, 3)
        gt, pred = img_gt, img_pred
        gt, pred = (gt - 0.5) * 2., (pred - 0.5) * 2.
        gt, pred = gt.permute([0, 3, 1, 2]), pred.permute([0, 3, 1, 2])
        lpips_fine += ref(pred, gt).reshape(-1)
        assert torch.equal(fn.seen[0][i_patch], pred[0].detach()) and torch.equal(fn.seen[1][i_patch], gt[0])
    lpips_fine = lpips_fine / 4
    d_want, = torch.autograd.grad(lpips_fine[0], rgb)
    assert got.shape == (1,) and torch.allclose(got, lpips_fine, rtol=1e-6, atol=0) and torch.allclose(d_got, d_want, rtol=1e-5, atol=1e-9)
    assert (d_got[4 * 256:] == 0).all()
    assert patch_lpips(rgb, target_s, fn, n_patches=2).item() == pytest.approx(float(ref(fn.seen[0][:2], fn.seen[1][:2]).sum()) / 4, rel=1e-6)
    with pytest.raises(ValueError):
        patch_lpips(rgb[:100], target_s[:100], fn)
    with pytest.raises(ValueError):
        patch_lpips(rgb, target_s, fn, patch_size=8)
