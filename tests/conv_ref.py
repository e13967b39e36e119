"""fp64 references of the convolution forms the plans launch (tests/test_ops_forms_gpu.py, tests/test_ops_gpu.py), and the
destination buffers those tests hand to the kernel-level hook.  Everything is NHWC, as the library's tensors are; the arithmetic is
torch's own conv2d / conv_transpose2d in float64 on whatever device the inputs live on."""
import torch
import torch.nn.functional as F

SENTINEL = 1e30                  # fills the input channels past Cin: one stray read ruins the output
PREFILL_BITS = 0x7FC0BEEF       # a quiet NaN with a payload no kernel produces (fits a positive int32)


def pad_input(x, in_ld):
    """x [B,H,W,Cin] -> [B,H,W,in_ld]: the channels past Cin hold SENTINEL."""
    B, H, W, Cin = x.shape
    assert in_ld >= Cin
    out = torch.full((B, H, W, in_ld), SENTINEL, dtype=x.dtype, device=x.device)
    out[..., :Cin] = x
    return out


def conv_forms_ref(x, w, b=None, stride=1, pad=0, act=0, gate=None, resid=None, deconv=False, cin=None):
    """float64 NHWC result of one launch.  x [B,H,W,in_ld] (only the first `cin` channels are the layer's input; default: the
    weight's input channels), w [Cout,Cin,KH,KW] (deconv: [Cin,Cout,2,2], ConvTranspose2d k2 s2), gate [B,Cin] multiplies the input
    per sample and channel before the conv, act 0 none / 1 relu / 2 swish, resid [B,OH,OW,>=Cout] is added after the activation
    (its first Cout channels)."""
    if cin is None:
        cin = w.shape[0] if deconv else w.shape[1]
    xd = x[..., :cin].double()
    if gate is not None:
        xd = xd * gate.double()[:, None, None, :]
    xd = xd.permute(0, 3, 1, 2)
    bd = b.double() if b is not None else None
    if deconv:
        y = F.conv_transpose2d(xd, w.double(), bd, stride=2)
    else:
        y = F.conv2d(xd, w.double(), bd, stride=stride, padding=pad)
    if act == 1:
        y = F.relu(y)
    elif act == 2:
        y = y * torch.sigmoid(y)
    y = y.permute(0, 2, 3, 1)
    if resid is not None:
        y = y + resid[..., :y.shape[3]].double()
    return y.contiguous()


def make_dst(B, OH, OW, ld, device):
    """A destination [B,OH,OW,ld] pre-filled with PREFILL_BITS, followed in the same allocation by one guard row of ld floats
    with the same fill.  Returns (whole flat buffer, the [B,OH,OW,ld] view)."""
    n = B * OH * OW * ld
    flat = torch.empty(n + ld, dtype=torch.float32, device=device)
    flat.view(torch.int32).fill_(PREFILL_BITS)
    return flat, flat[:n].view(B, OH, OW, ld)


def untouched_outside(flat, view, coff, n):
    """True when every float of the buffer outside channels [coff, coff + n) of the view's rows - the guard row included - still
    holds the pre-fill, bit for bit."""
    bits = flat.view(torch.int32)
    want = PREFILL_BITS
    rows = view.shape[0] * view.shape[1] * view.shape[2]
    ld = view.shape[3]
    body = bits[:rows * ld].view(rows, ld)
    ok = bool((body[:, :coff] == want).all()) and bool((body[:, coff + n:] == want).all())
    return ok and bool((bits[rows * ld:] == want).all())


def rel_err(out, ref):
    """max |out - ref| relative to the reference's max, in float64."""
    return ((out.double() - ref).abs().max() / ref.abs().max()).item()
