"""Laws every weight format of ops/quant.py (FORMATS) obeys, through its 2-D and its expert
container: slicing commutes with dequantization, an expert is the 2-D weight of its codes, views
stay views, and the loader's fuse helper and checkpoint form keep codes and scales bit for bit.
N = 8, K = 128, E = 3: the smallest shapes with a scale-block boundary (32), a half-byte
boundary (odd columns) and an expert boundary."""
import pytest
import torch

from aws_k8s_ansible_provisioner_amd.models.transformer import _checkpoint_proj, _fuse_rows
from aws_k8s_ansible_provisioner_amd.ops.quant import (FORMATS, QuantExperts, QuantWeight,
                                                       quantize_experts)

E, N, K = 3, 8, 128
pytestmark = pytest.mark.parametrize("fmt", list(FORMATS.values()), ids=list(FORMATS))


def _same(a, b) -> bool:
    """Same container class, codes and scales bit for bit."""
    return type(a) is type(b) and torch.equal(a.q, b.q) and torch.equal(a.scale, b.scale)


def _experts(fmt):
    w = torch.randn(E, N, K, generator=torch.Generator().manual_seed(3)) * 0.05
    w[1, 2] = 0.0          # an all-zero channel
    w[2, 5, 32:64] = 0.0   # an all-zero scale block
    return quantize_experts(w, fmt), w


def test_containers_and_table(fmt):
    we, w = _experts(fmt)
    assert type(we) is fmt.Experts and isinstance(we, QuantExperts) and we.fmt is fmt
    assert type(we[0]) is fmt.Weight and isinstance(we[0], QuantWeight) and we[0].fmt is fmt
    assert tuple(we.shape) == (E, N, K) and we.numel() == E * N * K and we.dim() == 3
    assert we.q.shape == (E, N, K // fmt.per_byte) and we.q.dtype == torch.uint8
    assert tuple(we.scale.shape) == fmt.scale_shape((E, N), K) and we.scale.dtype == fmt.scale_dtype
    assert we.nbytes == we.q.numel() + we.scale.numel() * we.scale.element_size()
    assert torch.isfinite(we.float()).all()


def test_slice_then_float_is_float_then_slice(fmt):
    we, _ = _experts(fmt)
    f3, w2 = we.float(), we[1]
    f2 = w2.float()
    assert torch.equal(f2, f3[1])
    assert torch.equal(w2[2:7].float(), f2[2:7])                # rows
    assert torch.equal(w2[:, 32:96].float(), f2[:, 32:96])      # whole scale blocks
    assert torch.equal(w2[1:, 96:].float(), f2[1:, 96:])
    assert torch.equal(we[1:3].float(), f3[1:3])                # experts
    assert torch.equal(we[:, 2:7].float(), f3[:, 2:7])          # channels of every expert
    assert torch.equal(we[:, :, 32:96].float(), f3[:, :, 32:96])
    assert torch.equal(we[2, 1:5, 64:].float(), f3[2, 1:5, 64:])
    for cols in (slice(16, 48), slice(3, 35)):  # inside a scale block; on a half byte
        if fmt.block:
            with pytest.raises(ValueError, match="multiples of 32"):
                w2[:, cols]
            with pytest.raises(ValueError, match="multiples of 32"):
                we[:, :, cols]
        else:
            assert torch.equal(w2[:, cols].float(), f2[:, cols])
            assert torch.equal(we[:, :, cols].float(), f3[:, :, cols])
    with pytest.raises(TypeError):
        w2[0]
    with pytest.raises(TypeError):
        we[:, 0]
    with pytest.raises(IndexError):
        we[0, :, :, :]


def test_an_expert_is_the_2d_weight_of_its_codes(fmt):
    we, w = _experts(fmt)
    for e in range(E):
        assert _same(we[e], fmt.Weight(we.q[e], we.scale[e]))
        assert _same(we[e], fmt.quantize(w[e]))


def test_flat_is_a_view_and_to_keeps_the_class(fmt):
    we, _ = _experts(fmt)
    flat = we.flat()
    assert type(flat) is fmt.Weight and tuple(flat.shape) == (E * N, K)
    assert flat.q.data_ptr() == we.q.data_ptr() and flat.scale.data_ptr() == we.scale.data_ptr()
    assert torch.equal(flat.float().view(E, N, K), we.float())
    for w in (we, we[0]):
        assert _same(w.to("cpu"), w)
        assert repr(w) == f"{type(w).__name__}(shape={tuple(w.shape)}, device=cpu)"


def test_fuse_rows_keeps_codes_and_scales(fmt):
    we, _ = _experts(fmt)
    a, b = we[0], we[1][:5]
    fused = _fuse_rows([a, b])
    assert type(fused) is fmt.Weight and tuple(fused.shape) == (N + 5, K)
    assert torch.equal(fused.q, torch.cat([a.q, b.q])) and torch.equal(fused.scale,
                                                                        torch.cat([a.scale, b.scale]))
    assert _same(fused[:N], a) and _same(fused[N:], b)
    # a plain part next to a quantized one: both are dequantized, exactly
    mixed = _fuse_rows([a, b.float()])
    assert torch.equal(mixed, torch.cat([a.float(), b.float()]))


def test_export_form_loads_back_equal(fmt):
    we, _ = _experts(fmt)
    w = we[2]
    sd = {}
    sd["p.weight"], sd["p.weight_scale"] = w.hf_export()
    assert sd["p.weight"].dtype in fmt.ckpt_dtypes
    assert sd["p.weight"].data_ptr() != w.q.data_ptr()  # copies: a checkpoint owns its tensors
    assert _same(_checkpoint_proj(sd, "p", fmt.name), w)
    other = next(f for f in FORMATS.values() if f is not fmt)
    with pytest.raises(ValueError, match=f"--quantization {fmt.name}"):
        _checkpoint_proj(sd, "p", other.name)
