"""float64 restatement of the decode GEMVs (csrc/gemm_skinny.hip: gar_gemm at M <= 64 and gar_gemm_w8) for the tests, with a bound
on |kernel - restatement| PER ELEMENT. The bound comes from the arithmetic the ABI states — 16-bit operands multiplied exactly,
f32 accumulation in some order, the norm's f32 rstd, the epilogue in f32, ONE rounding to the 16-bit output — never from what a
kernel gives:
    summation order   K * 2^-24 * sum_k |x w|      (every f32 add of a sum of K terms, in any order)
    rsqrtf            2^-22 * |acc|
    SwiGLU            the two errors above carried through silu(gate) * up, plus 1e-5 for the kernel's fast exp
    output rounding   OUT_EPS * |result|             (bf16: 2^-8, fp16: 2^-11; a split-K partial is f32 and has none)
The weight is a 16-bit tensor [N, K] (scale 1) or the pair (e4m3 bytes uint8 [N, K], f32 row scales [N]) of the fp8-weight form.
torch is imported at module level, the GPU library nowhere: the epilogue codes come from gar_amd.hip inside the functions."""
import torch

OUT_EPS = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
OUT_TINY = {torch.bfloat16: 2.0 ** -133, torch.float16: 2.0 ** -24}     # spacing of the subnormal numbers


def weight_f64(w):
    """the weight operand as (float64 [N, K] without its row scales, float64 row scales [N] or None)"""
    if isinstance(w, (tuple, list)):
        q, s = w
        return q.view(torch.float8_e4m3fn).double(), s.double()
    return w.double(), None


def gemv_ref(x, w, epi, res=None, norm_w=None, folded=False, eps=1e-5, dt=torch.bfloat16, bias=None):
    """f64 restatement of gar_gemm (M <= 64) / gar_gemm_w8 -> (reference, bound on |kernel - reference|), both [M, N] (SwiGLU:
    [M, N / 2]; the weight rows interleave gate and up in groups of 16)"""
    import torch.nn.functional as Fn
    from gar_amd import hip
    xd = x.double()
    K = x.shape[1]
    rstd = None
    if norm_w is not None:          # NORM 1: the operand is x * g rounded to the 16-bit type, rstd comes from x
        xd = (x.float() * norm_w.float()).to(dt).double()
    if norm_w is not None or folded:
        rstd = torch.rsqrt((x.double() ** 2).mean(1, keepdim=True) + eps)
    wd, s = weight_f64(w)
    acc = xd @ wd.T
    mag = xd.abs() @ wd.abs().T
    if s is not None:
        acc, mag = acc * s[None, :], mag * s[None, :]
    if rstd is not None:
        acc, mag = acc * rstd, mag * rstd
    err = mag * (K * 2.0 ** -24) + acc.abs() * 2.0 ** -22              # summation order; rsqrtf
    if epi == hip.EPI_SWIGLU:
        N = acc.shape[1]
        a4, m4 = acc.view(-1, N // 32, 2, 16), err.view(-1, N // 32, 2, 16)
        gate, up = a4[:, :, 0], a4[:, :, 1]
        out = (Fn.silu(gate) * up).reshape(acc.shape[0], -1)
        # d(silu(g) u) <= 1.1 |u| dg + |silu(g)| du, plus the kernel's fast exp
        err = (1.1 * up.abs() * m4[:, :, 0] + Fn.silu(gate).abs() * m4[:, :, 1]).reshape(acc.shape[0], -1) + out.abs() * 1e-5
        acc = out
    if epi == hip.EPI_RES:
        acc = acc + res.double()
    if epi == hip.EPI_BIAS:
        acc = acc + bias.double()[None, :]
    return acc, err + acc.abs() * OUT_EPS[dt] + 1e-30


def rmsnorm_ref(h, g, eps=1e-5, dt=torch.bfloat16):
    """f64 RMSNorm of the 16-bit rows ``h`` with gain ``g`` as gar_rmsnorm / gar_splitk_residual_rmsnorm state it -> (reference,
    bound). The ABI rounds TWICE (HF LlamaRMSNorm: weight * hidden.to(dtype)): n = round(h * rstd), y = round(g * n). So the bound
    carries two output roundings (1 + e)^2 - 1, the rsqrtf, the f32 sum of D squares in any order (D * 2^-24 of the sum, half of
    it on rstd) and the few f32 multiplies. Below the smallest normal number a rounding is absolute, half of OUT_TINY: the first
    one reaches the output times |g|, the second as it is (fp16 only in practice: an element of h near 1e-5 of its row's rms)."""
    hd = h.double()
    D = h.shape[1]
    e = OUT_EPS[dt]
    ref = hd * torch.rsqrt((hd ** 2).mean(1, keepdim=True) + eps) * g.double()[None, :]
    tiny = 0.5 * OUT_TINY[dt] * (g.double().abs()[None, :] + 1)
    return ref, ref.abs() * (2 * e + e * e + 2.0 ** -22 + D * 2.0 ** -25 + 4 * 2.0 ** -24) + tiny


def row_gain(out, ref):
    """per row m: <out_m, ref_m> / <ref_m, ref_m> in f64 — the scale a row carries against its reference (1 when exact). A
    row's rstd that lost a piece of its sum of squares shows here, where it is far below the rounding of a single element."""
    o, r = out.double(), ref.double()
    return (o * r).sum(1) / (r * r).sum(1)
