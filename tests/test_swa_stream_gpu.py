"""The streaming route of mmr_swin_window_attention (csrc/swin_wattn.hip; MMR_PIN_SWA = 1) against the
gather kernel (MMR_PIN_SWA = 0): the arithmetic is the same operation for operation, so the outputs are
compared bit for bit; one case per Swin stage is also held to the oracle restatement (rel_err < 2e-2, the
rule of test_towers_gpu.py::test_swin_window_attention).

Launch rule of the streaming route (include/mmr.h): persistent workgroups of STREAM_WAVES waves,
min(CUs, ceil(units / STREAM_WAVES)) of them, units = images x windows x head pairs in (window, head
pair)-major order; wave g of the G = workgroups x STREAM_WAVES takes units [g units / G, (g + 1) units / G).
The automatic route takes the streaming kernel from 3 units per wave up, so the small cases here pin it."""
import pytest
import torch

from mmr_amd import ops
from oracle import towers as otw

pytestmark = pytest.mark.gpu
DEV = "cuda"
WS = 7
STREAM_WAVES = 4


def _bits(t):
    return t.contiguous().view(torch.int16)


def _inputs(B, hw, heads, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, hw, hw, 3 * heads * 32, generator=g).to(torch.bfloat16)
    table = torch.randn((2 * WS - 1) ** 2, heads, generator=g)
    return qkv, table


def _both(qkv, table, hw, heads, shift, ws=WS):
    qd = qkv.to(DEV)
    bias = ops.swin_attn_bias(table.to(DEV), heads, ws, hw, shift)
    with ops.pinned(ops.PIN_SWA, 0):
        y0 = ops.swin_window_attention(qd, bias, hw, heads, ws, shift)
    with ops.pinned(ops.PIN_SWA, 1):
        y1 = ops.swin_window_attention(qd, bias, hw, heads, ws, shift)
    torch.cuda.synchronize()
    return y0, y1


def _ref(qkv, table, H, heads, ws, shift):
    """timm WindowAttention + cyclic shift on the bf16 operands, f32 (test_towers_gpu.py's restatement)."""
    B, C, N, hd = qkv.shape[0], qkv.shape[-1] // 3, ws * ws, 32
    x = qkv.float()
    if shift:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    win = otw.window_partition(x, ws).view(-1, N, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = win[0] * hd ** -0.5, win[1], win[2]
    a = q @ k.transpose(-2, -1)
    a = a + table[otw.relative_position_index(ws).view(-1)].view(N, N, heads).permute(2, 0, 1)[None]
    if shift:
        m = otw.shift_mask(H, H, ws, shift)
        a = (a.view(-1, m.shape[0], heads, N, N) + m[None, :, None]).view(-1, heads, N, N)
    o = (a.softmax(-1) @ v).transpose(1, 2).reshape(-1, ws, ws, C)
    o = otw.window_reverse(o, ws, H, H)
    if shift:
        o = torch.roll(o, shifts=(shift, shift), dims=(1, 2))
    return o.reshape(B, H, H, C)


# the Swin-T stages 2-4, and two heads at hw = 7 / 14: 1, 2, 5 / 4, 8, 20 units, fewer than or no
# multiple of a workgroup's waves
GEOS = [(28, 6, 0), (28, 6, 3), (14, 12, 0), (14, 12, 3), (7, 24, 0), (7, 2, 0), (14, 2, 3)]


@pytest.mark.parametrize("B", [1, 2, 5])
@pytest.mark.parametrize("hw,heads,shift", GEOS)
def test_stream_bit_identical(hw, heads, shift, B):
    qkv, table = _inputs(B, hw, heads, 1000 * hw + 10 * heads + shift + B)
    y0, y1 = _both(qkv, table, hw, heads, shift)
    assert torch.isfinite(y1.float()).all()
    assert torch.equal(_bits(y1), _bits(y0))


@pytest.mark.parametrize("hw,heads,shift", [(28, 6, 3), (14, 12, 3), (7, 24, 0)])
def test_stream_vs_oracle(hw, heads, shift):
    qkv, table = _inputs(2, hw, heads, hw + heads + shift)
    ref = _ref(qkv, table, hw, heads, WS, shift)
    y1 = _both(qkv, table, hw, heads, shift)[1].float().cpu().reshape(ref.shape)
    rel = (y1 - ref).abs().max().item() / max(ref.abs().max().item(), 1e-12)
    print(f"hw {hw} heads {heads} shift {shift}: rel_err {rel:.3e}")
    assert rel < 2e-2


@pytest.mark.parametrize("hw,heads,shift", [(7, 24, 0), (14, 12, 3)])
def test_stream_walk(hw, heads, shift):
    """Every wave takes two or three units (units = 2 G + G / 2 + 3, rounded up to whole images), and a
    wave's range crosses (window, head pair) boundaries, where it reloads its bias rows: a late or missing
    prefetch would read the previous unit's image, a missed reload the previous pair's bias."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = cus * STREAM_WAVES
    per_image = (hw // WS) ** 2 * (heads // 2)
    units = 2 * G + G // 2 + 3
    B = -(-units // per_image)
    assert -(-B * per_image // STREAM_WAVES) >= cus  # the launch rule's min() takes the CU count
    assert 2 * G < B * per_image < 3 * G
    qkv, table = _inputs(B, hw, heads, 7 * hw + heads)
    y0, y1 = _both(qkv, table, hw, heads, shift)
    assert torch.equal(_bits(y1), _bits(y0))


def test_stream_automatic():
    """Unpinned, at the smallest size the automatic route sends to the streaming kernel (3 units per
    wave: stage 4, hw = 7 / 24 heads, at 64 images per 256 waves), the same bits as the gather kernel."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    hw, heads = 7, 24
    B = -(-3 * cus * STREAM_WAVES // (heads // 2))
    qkv, table = _inputs(B, hw, heads, 99)
    qd = qkv.to(DEV)
    bias = ops.swin_attn_bias(table.to(DEV), heads, WS, hw, 0)
    with ops.pinned(ops.PIN_SWA, 0):
        y0 = ops.swin_window_attention(qd, bias, hw, heads, WS, 0)
    y = ops.swin_window_attention(qd, bias, hw, heads, WS, 0)
    torch.cuda.synchronize()
    assert torch.equal(_bits(y), _bits(y0))


@pytest.mark.parametrize("ws,hw,shift,heads", [(8, 16, 3, 3), (4, 8, 1, 1), (7, 56, 3, 3)])
def test_stream_declined_geometry(ws, hw, shift, heads):
    """Windows other than 7 x 7 and odd head counts (stage 1: 3 heads) stay on the gather kernel: pinning
    the streaming route still succeeds and gives the same bits."""
    g = torch.Generator().manual_seed(100 * ws + 10 * shift + heads)
    qkv = torch.randn(2, hw, hw, 3 * heads * 32, generator=g).to(torch.bfloat16)
    table = torch.randn((2 * ws - 1) ** 2, heads, generator=g)
    y0, y1 = _both(qkv, table, hw, heads, shift, ws=ws)
    assert torch.isfinite(y1.float()).all()
    assert torch.equal(_bits(y1), _bits(y0))
