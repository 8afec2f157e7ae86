"""az_amd.state_dict_blob on CPU tensors: a module's state_dict as the engine's canonical parameter blob --
the entries in order, num_batches_tracked skipped, float32, optionally written into a caller's tensor."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")


def _module():
    nn = torch.nn
    torch.manual_seed(3)
    m = nn.Sequential(nn.Conv2d(3, 4, 3, bias=False), nn.BatchNorm2d(4), nn.Conv2d(4, 2, 1, bias=True), nn.BatchNorm2d(2),
                      nn.Flatten(), nn.Linear(8, 5))
    with torch.no_grad():
        for bn in (m[1], m[3]):
            bn.running_mean.uniform_(-1, 1)
            bn.running_var.uniform_(0.5, 2)
            bn.num_batches_tracked.fill_(17)
    return m


def _expected(sd):
    return np.concatenate([v.detach().numpy().astype(np.float32).ravel() for k, v in sd.items()
                           if not k.endswith("num_batches_tracked")])


def test_state_dict_blob_concatenates_in_order():
    import az_amd
    sd = _module().state_dict()
    assert any(k.endswith("num_batches_tracked") for k in sd)
    blob = az_amd.state_dict_blob(sd)
    assert blob.dtype == torch.float32 and blob.dim() == 1 and blob.is_contiguous() and not blob.is_cuda
    exp = _expected(sd)
    assert blob.numel() == exp.size == 3 * 4 * 9 + 4 * 4 + (4 * 2 + 2) + 4 * 2 + (8 * 5 + 5)
    assert np.array_equal(blob.numpy().view(np.uint32), exp.view(np.uint32))
    # the layout in words: conv weight, then BN weight / bias / running_mean / running_var
    assert np.array_equal(blob[:108].numpy(), sd["0.weight"].numpy().ravel())
    assert np.array_equal(blob[108:124].numpy(), np.concatenate([sd["1." + k].numpy() for k in
                                                                 ("weight", "bias", "running_mean", "running_var")]))
    assert 17.0 not in blob.tolist()


def test_state_dict_blob_writes_into_out():
    import az_amd
    m = _module()
    sd = m.state_dict()
    out = torch.full((_expected(sd).size,), 7.0)
    got = az_amd.state_dict_blob(sd, out=out)
    assert got is out
    assert np.array_equal(out.numpy(), _expected(sd))
    with torch.no_grad():
        m[5].bias.add_(1.0)
    az_amd.state_dict_blob(m.state_dict(), out=out)                  # a refresh into the same tensor
    assert np.array_equal(out.numpy(), _expected(m.state_dict()))
    for bad in (torch.zeros(out.numel() + 1), torch.zeros(out.numel(), dtype=torch.float64),
                torch.zeros(2 * out.numel())[::2]):
        with pytest.raises(ValueError):
            az_amd.state_dict_blob(sd, out=bad)


def test_state_dict_blob_converts_other_dtypes():
    import az_amd
    sd = {"a": torch.arange(4, dtype=torch.float64).reshape(2, 2), "b.num_batches_tracked": torch.tensor(3),
          "c": torch.tensor([1.5], dtype=torch.float16)}
    assert az_amd.state_dict_blob(sd).tolist() == [0.0, 1.0, 2.0, 3.0, 1.5]
