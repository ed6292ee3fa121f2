"""The transformer branches (models/HDenseFormer.py:33-145) restated STAGE BY STAGE, as the plan stores them, for the
teacher-forced checks of test_gpu_transformer_rounding.py: every function maps the tensors one stage reads to the tensors
it writes, in whatever float type its arguments have (fp64 for the reference, fp32 for the accumulation allowance), so a
stage can be evaluated on the DEVICE'S OWN inputs to it and compared with the device's output of that stage alone.

The arithmetic is the oracle's (oracle/hdf_oracle.py: _layer_norm, _dense_forward, _conv, Dropper; the dropout site ids of
oracle/detgen.py) wherever the oracle has the piece as a function of its own.  Two pieces it has only fused with their
neighbours are written out here -- the softmax core between to_qkv and to_out (attn_core: the plan stores qkv, the merged
heads and the log-sum-exp) and the inside of DenseForward between its two dropouts (dense_parts: the tapes hold it) -- and
tests/test_tf_ref_cpu.py pins both, composed, to oracle.hdf_oracle.transformer_branch and to autograd through it.

Tensors of one modality are [B, N, width] (the dropout element index is the flat index of that tensor).  Stage boundaries
(csrc/transformer.h, api_ops.hip:save_ptrs, plan.hip:hdf_plan_layout; K = DM + 32 l):

  forward   x, patch weight / bias / position -> F[0][:, 0:DM]                                  patch_embed
            F[b][:, 0:K] -> h0 -> (t = LN1 h0) -> qkv                                           pre
            qkv -> ob, lse                                                                     attn_core
            ob, h0 -> h1 ; h1 -> h2 ; h2 -> F[b][:, K:K+32]                                     post_h1, ff, ff
            F[b] -> F[b+1][:, 0:DM] or attnall                                                  block_out
  backward  branch_backward: the layer tapes (TF_T_DQ, _T, _DH0, _P1, _P0, _DGO), the out-layer tapes (do | f | dz) and
            the gradient of block 0's input, each from the tape segments upstream of it; param_grads: every parameter
            gradient of a branch as the contraction / column sum of tape operands it is (TfWgradEntry, colsum_atomic).
"""
import torch
import torch.nn.functional as F

from hdf_rt._lib import BF16, F16, F32
from oracle import detgen
from oracle import hdf_oracle as orc

TDT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
G = orc.GROWTH               # 32: width of a dense layer
TAPE_W = 576                 # TF_TAPE_W
T_DQ, T_T, T_DH0, T_P1, T_P0, T_DGO = 0, 96, 128, 160, 352, 544     # segment columns of a layer tape (transformer.h)
SAVE_W = 232                 # floats per token of a layer's saved tensors
SAVE_SEG = (("h0", 0, 32), ("qkv", 32, 96), ("ob", 128, 32), ("lse", 160, 8), ("h1", 168, 32), ("h2", 200, 32))


# The accumulation allowance of a stage is FACTOR x max|stage in torch fp32 - stage in torch fp64| on the same inputs: a
# property of the reference alone.  4 unless the stage is listed (test_gpu_transformer_rounding.py's docstring has the
# measured ratios and the hardware intrinsic every larger factor is attributed to).
FACTOR = {}


def acc_of(stage, ref32, ref64, alt64=None):
    """alt64: the fp64 reference with the kernel-formed 16-bit operands (P, dS) formed in fp32 instead of fp64 -- a rounding
    of such an operand that flips between the two is no error of the kernel"""
    acc = FACTOR.get(stage, 4.0) * float((ref32.double() - ref64).abs().max())
    if alt64 is not None:
        acc += float((alt64 - ref64).abs().max())
    return acc


def group_accs(stage, ref32, ref64, width=0, alt64=None):
    """[(columns, acc)]: the allowance per group of `width` columns (a head; 0: the whole tensor).  One head may be a
    thousand times smaller than the others, so every head gets an allowance of its own scale; but a head of a few tokens
    is a small sample -- its fp32 and fp64 evaluations can agree by accident -- so a head's spread is taken as at least
    the worst RELATIVE spread of all heads (spread / largest reference of the head) times its own largest reference."""
    if not width:
        return [(slice(None), acc_of(stage, ref32, ref64, alt64))]
    cols = [slice(c, c + width) for c in range(0, ref64.shape[-1], width)]
    spread = [float((ref32[..., s].double() - ref64[..., s]).abs().max()) for s in cols]
    scale = [float(ref64[..., s].abs().max()) for s in cols]
    rel = max([sp / sc for sp, sc in zip(spread, scale) if sc > 0] or [0.0])
    out = []
    for s, sp, sc in zip(cols, spread, scale):
        acc = FACTOR.get(stage, 4.0) * max(sp, rel * sc)
        if alt64 is not None:
            acc += float((alt64[..., s] - ref64[..., s]).abs().max())
        out.append((s, acc))
    return out


def lp_round(t, dtype):
    """a value the kernel holds in fp32 and hands to the matrix core as a 16-bit operand: ONE rounding to nearest-even from
    fp32, exact in the float type of `t` afterwards; F32: unchanged"""
    if dtype == F32:
        return t
    return t.float().to(TDT[dtype]).to(t.dtype)


def layer_prefix(m, b, l):
    return "attns.%d.blocks.%d.0.layers.%d" % (m, b, l)


def block_prefix(m, b):
    return "attns.%d.blocks.%d.0" % (m, b)


def mask(drop, site, shape, dtype):
    """the dropout multiplier (0 or 1 / (1 - p); ones in eval mode) of a site for a [B, N, width] tensor"""
    return drop(torch.ones(shape, dtype=dtype), site)


# ------------------------------------------------------------------------------------------------ forward stages
def patch_embed(vol, sd, m, drop, dtype=F32):
    """vol [B, 1, D, H, W] (2-D model: [B, 1, H, W]) -> F[0][:, 0:DM] as [B, N, DM].  16-bit plans: x and the weight are
    rounded to the storage type first (patch_embed_fwd2_kernel<1|2>), bias and position stay as they are"""
    p = "attns.%d" % m
    t = orc._conv(lp_round(vol, dtype), lp_round(sd[p + ".patch_embeddings.weight"], dtype), None, stride=orc.PATCH)
    tok = t.flatten(2).transpose(1, 2) + sd[p + ".patch_embeddings.bias"]
    return drop(tok + sd[p + ".position_embeddings"], detgen.site_emb(m))


def qkv_of(h0, sd, lp):
    """h0 -> (t = LN1(h0), qkv)"""
    t = orc._layer_norm(h0, sd, lp + ".1.norm")
    return t, F.linear(t, sd[lp + ".1.fn.to_qkv.weight"])


def pre(Fk, sd, lp):
    """F[b][:, 0:K] -> (h0, t = LN1(h0), qkv)"""
    h0 = F.linear(Fk, sd[lp + ".0.weight"], sd[lp + ".0.bias"])
    return (h0,) + qkv_of(h0, sd, lp)


def heads(x):
    """[B, N, 8 * w] -> [B, 8, N, w]"""
    b, n, c = x.shape
    return x.reshape(b, n, orc.HEADS, c // orc.HEADS).permute(0, 2, 1, 3)


def merge(x):
    """[B, 8, N, w] -> [B, N, 8 * w]"""
    b, h, n, w = x.shape
    return x.permute(0, 2, 1, 3).reshape(b, n, h * w)


def attn_core(qkv):
    """qkv [B, N, 96] -> ob [B, N, 32] (heads merged, before to_out), lse [B, N, 8] (natural log)"""
    q, k, v = [heads(t) for t in qkv.split(G, dim=-1)]
    s = torch.matmul(q, k.transpose(-1, -2)) * (q.shape[-1] ** -0.5)
    return merge(torch.matmul(torch.softmax(s, dim=-1), v)), torch.logsumexp(s, dim=-1).permute(0, 2, 1)


def attn_inputs(nseq, N, seed, peaked):
    """qkv [nseq, N, 96] / d_ob [nseq, N, 32] of the operator-level attention cases: head 7's v and d_ob a thousand times
    smaller than the others'; `peaked`: scores up to about 60 around a common offset of +40 per row (every q has the
    component 8 and every k the component 10 on the head's last axis: 0.5 * 8 * 10 on every score)"""
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(nseq, N, 96, generator=g) * 1.5
    d_ob = torch.randn(nseq, N, 32, generator=g)
    if peaked:
        q, k = qkv[..., :32].reshape(nseq, N, 8, 4), qkv[..., 32:64].reshape(nseq, N, 8, 4)      # (views)
        q *= 2.2
        k *= 2.2
        q[..., 3] = 8.0
        k[..., 3] = 10.0
    qkv[..., 64 + 28:] *= 1e-3
    d_ob[..., 28:] *= 1e-3
    return qkv, d_ob


def post_h1(ob, h0, sd, lp, drop, site):
    return drop(F.linear(ob, sd[lp + ".1.fn.to_out.0.weight"], sd[lp + ".1.fn.to_out.0.bias"]), site) + h0


def ff(h, sd, lp, drop, site_a, site_b):
    """DenseForward(LN2(h)) without the residual"""
    return orc._dense_forward(orc._layer_norm(h, sd, lp + ".2.norm"), sd, lp + ".2.fn", drop, site_a, site_b)


def block_out(Fb, sd, bp, drop, m, b):
    return orc._dense_forward(Fb, sd, bp + ".out_layer", drop, detgen.site_id(m, b, detgen.LAYER_OUT, detgen.KIND_OUT_A),
                              detgen.site_id(m, b, detgen.LAYER_OUT, detgen.KIND_OUT_B))


def layer_forward(Fk, sd, m, b, l, drop):
    """one dense layer from its input columns: every tensor the plan saves, and the feature it appends"""
    lp = layer_prefix(m, b, l)

    def s(kind):
        return detgen.site_id(m, b, l, kind)
    h0, t, qkv = pre(Fk, sd, lp)
    ob, lse = attn_core(qkv)
    h1 = post_h1(ob, h0, sd, lp, drop, s(detgen.KIND_ATTN_OUT))
    h2 = ff(h1, sd, lp, drop, s(detgen.KIND_FF1_A), s(detgen.KIND_FF1_B)) + h1
    feat = ff(h2, sd, lp, drop, s(detgen.KIND_FF2_A), s(detgen.KIND_FF2_B))
    return dict(h0=h0, qkv=qkv, ob=ob, lse=lse, h1=h1, h2=h2, feat=feat)


def branch_forward(vol, sd, m, nb, drop, dtype=F32):
    """the stages composed: {"F": [nb] x [B, N, DM + 128], "save": [nb][4] dicts, "out": [B, N, DM]}"""
    x = patch_embed(vol, sd, m, drop, dtype)
    Fs, saves = [], []
    for b in range(nb):
        feats, sv = [x], []
        for l in range(orc.LAYERS):
            r = layer_forward(torch.cat(feats, 2), sd, m, b, l, drop)
            feats.append(r.pop("feat"))
            sv.append(r)
        Fs.append(torch.cat(feats, 2))
        saves.append(sv)
        x = block_out(Fs[-1], sd, block_prefix(m, b), drop, m, b)
    return {"F": Fs, "save": saves, "out": x}


# ------------------------------------------------------------------------------------------------ backward stages
def dense_parts(u, sd, p, drop, site_a):
    """the inside of DenseForward up to its second dropout: z = net.0(u), f = dropout(gelu(z)), g = net.3(f)"""
    z = F.linear(u, sd[p + ".net.0.weight"], sd[p + ".net.0.bias"])
    f = drop(F.gelu(z), site_a)
    return z, f, F.linear(f, sd[p + ".net.3.weight"], sd[p + ".net.3.bias"])


def dense_front_bwd(u, dg, sd, p, drop, site_a):
    """dg = the gradient at g (the upstream gradient times the second dropout's mask) -> (f, dz): the tape's f | dz"""
    z = F.linear(u.detach(), sd[p + ".net.0.weight"], sd[p + ".net.0.bias"]).detach().requires_grad_(True)
    f = drop(F.gelu(z), site_a)
    g = F.linear(f, sd[p + ".net.3.weight"], sd[p + ".net.3.bias"])
    (dz,) = torch.autograd.grad(g, z, dg)
    return f.detach(), dz


def ln_linear_bwd(h, dy, sd, norm, weight):
    """gradient at h of Linear(LN(h)) for the gradient dy at the Linear's output (the bias does not matter)"""
    h = h.detach().requires_grad_(True)
    (dh,) = torch.autograd.grad(F.linear(orc._layer_norm(h, sd, norm), sd[weight]), h, dy)
    return dh


def attn_bwd_operands(qkv, ob, lse, dO):
    """P = exp(s - lse), D = dO v^T - delta, dS = P D of the attention backward, [B, 8, N, N], in the float type of qkv"""
    q, k, v = [heads(t) for t in qkv.split(G, dim=-1)]
    go, oo = heads(dO), heads(ob)
    s = torch.matmul(q, k.transpose(-1, -2)) * 0.5
    P = torch.exp(s - lse.permute(0, 2, 1).unsqueeze(-1))
    D = torch.matmul(go, v.transpose(-1, -2)) - (go * oo).sum(-1, keepdim=True)
    return P, D, P * D


def attn_bwd(qkv, ob, lse, dO, dtype=F32, form=None):
    """the attention backward as the kernels run it (attn_bwd_kernel; attn_bwd_lp_kernel for the 16-bit plans): from the
    SAVED ob and lse, P = exp(s - lse), delta = dO . ob, dS = P (dO v^T - delta); dq = 0.5 dS k, dk = 0.5 dS^T q,
    dv = P^T dO.  16-bit: the operands of those three accumulations -- dS, P, k, q, dO -- are rounded to the storage type
    (LpPack<LP>::four / ::one), scores, P and delta come from the unrounded fp32 tensors.  `form`: the float type P and dS
    are formed in before that rounding (default: that of qkv)."""
    wt = qkv.dtype
    ft = form or wt
    q, k, v = [heads(t) for t in qkv.split(G, dim=-1)]
    go = heads(dO)
    P, _, dS = attn_bwd_operands(qkv.to(ft), ob.to(ft), lse.to(ft), dO.to(ft))
    P, dS = lp_round(P, dtype).to(wt), lp_round(dS, dtype).to(wt)
    dq = 0.5 * torch.matmul(dS, lp_round(k, dtype))
    dk = 0.5 * torch.matmul(dS.transpose(-1, -2), lp_round(q, dtype))
    dv = torch.matmul(P.transpose(-1, -2), lp_round(go, dtype))
    return torch.cat([merge(dq), merge(dk), merge(dv)], dim=-1)


def _ulp16(x, dtype):
    """spacing of the 16-bit storage type at |x| (hip_util.ulp_of)"""
    from hip_util import ulp_of
    return ulp_of(x, dtype)


def attn_bwd_ambiguity(qkv, ob, lse, dO, dtype, factor=4.0):
    """What two properties of the number formats may legitimately add to dqkv, per element, on top of the stage's
    accumulation allowance.  Returns [B, N, 96] (fp64).

    (1) The cancellation in D = dO v^T - delta, delta = dO . ob, every dtype.  Both are 4-term fp32 dot products, so D
    carries up to 4 * 2^-24 (sum |dO v| + sum |dO ob|) whatever D itself is -- with one key D is exactly zero and the fp32
    and fp64 evaluations on the CPU agree to the last bit, yet no fp32 kernel can.  dS = P D inherits P times that; it
    reaches dq and dk through |k| and |q|.

    (2) The 16-bit roundings of the operands the KERNEL forms (P, dS), 16-bit plans.  The kernel's fp32 P and dS differ
    from the fp64 ones by the error of an fp32 evaluation, so its rounding of an operand to the storage type can fall on the
    other side of a rounding tie than the reference's -- one 16-bit ulp of that operand times the other operand -- but
    ONLY for operands that lie that close to a tie.  The radius is the reference's own: tau_P = factor x the worst relative
    |P32 - P64| / P64 (fp32 and fp64 evaluation on the CPU), tau_D = factor x max |D32 - D64| + the bound of (1); an
    operand is ambiguous when its distance to the nearest tie is within tau_P |P| (P), tau_P |dS| + tau_D P (dS = P D).
    The allowance is the sum over the ambiguous operands of ulp16(operand) x |other operand|.  About one operand in fifty
    is ambiguous with bf16 at scores of tens; a rounding that truncates moves EVERY operand and stays far outside
    (tests/test_tf_ref_cpu.py)."""
    args64 = [t.double() for t in (qkv, ob, lse, dO)]
    P, D, dS = attn_bwd_operands(*args64)
    q, k, v = [heads(t) for t in args64[0].split(G, dim=-1)]
    go, oo = heads(args64[3]), heads(args64[1])
    eD = 4.0 * 2.0 ** -24 * (torch.matmul(go.abs(), v.abs().transpose(-1, -2)) + (go * oo).abs().sum(-1, keepdim=True))
    eS = P * eD
    out = [0.5 * torch.matmul(eS, k.abs()), 0.5 * torch.matmul(eS.transpose(-1, -2), q.abs()), torch.zeros_like(q)]
    if dtype != F32:
        P32, D32, _ = attn_bwd_operands(*[t.float() for t in (qkv, ob, lse, dO)])
        live = P > 1e-30
        tau_p = factor * float(((P32.double() - P).abs() / P.clamp_min(1e-300))[live].max()) if bool(live.any()) else 0.0
        tau_d = factor * float((D32.double() - D).abs().max()) + eD

        def ambiguous(x, radius):
            u = _ulp16(x, dtype)
            dist = (torch.remainder(x.abs(), u) - 0.5 * u).abs()          # to the nearest tie of the storage type
            return torch.where(dist <= radius, u, torch.zeros_like(u))
        aP = ambiguous(P, tau_p * P)
        aS = ambiguous(dS, tau_p * dS.abs() + tau_d * P)
        qr, kr, gr = [lp_round(t, dtype).abs() for t in (q, k, go)]
        out[0] = out[0] + 0.5 * torch.matmul(aS, kr)
        out[1] = out[1] + 0.5 * torch.matmul(aS.transpose(-1, -2), qr)
        out[2] = out[2] + torch.matmul(aP.transpose(-1, -2), gr)
    return torch.cat([merge(t) for t in out], dim=-1)


def out_backward(Fb, up, sd, m, b, drop, devo=None):
    """the out-layer tape of block b from the gradient `up` of its output: do = up * mask | f | dz.  devo: the device's
    tape (teacher-forced: f and dz from ITS do)"""
    bp, o = block_prefix(m, b), {}
    o["do"] = up * mask(drop, detgen.site_id(m, b, detgen.LAYER_OUT, detgen.KIND_OUT_B), up.shape, up.dtype)
    o["f"], o["dz"] = dense_front_bwd(Fb, (devo or o)["do"], sd, bp + ".out_layer", drop,
                                      detgen.site_id(m, b, detgen.LAYER_OUT, detgen.KIND_OUT_A))
    return o


def layer_backward(sv, dfeat, sd, m, b, l, drop, dtype=F32, devt=None, form=None):
    """the tape of dense layer (b, l) from the gradient `dfeat` of the feature it appends and its saved tensors sv.
    devt: the device's tape of this layer (teacher-forced: every segment from ITS upstream segments).  Returns
    {"dq", "t", "dh0", "dgo", "p1": {"dg", "f", "dz", "u"}, "p0": {...}}; the layer adds dh0 W0 to dF[:, 0:K]."""
    lp, wt, shp = layer_prefix(m, b, l), dfeat.dtype, sv["h0"].shape
    t = {"p1": {}, "p0": {}}
    src = devt if devt is not None else t

    def site(kind):
        return detgen.site_id(m, b, l, kind)
    # second ff (on h2), then the first (on h1): dg | f | dz | u
    t["p1"]["dg"] = dfeat * mask(drop, site(detgen.KIND_FF2_B), shp, wt)
    t["p1"]["u"] = orc._layer_norm(sv["h2"], sd, lp + ".2.norm")
    t["p1"]["f"], t["p1"]["dz"] = dense_front_bwd(t["p1"]["u"], src["p1"]["dg"], sd, lp + ".2.fn", drop,
                                                  site(detgen.KIND_FF2_A))
    dh2 = ln_linear_bwd(sv["h2"], src["p1"]["dz"], sd, lp + ".2.norm", lp + ".2.fn.net.0.weight")
    t["p0"]["dg"] = dh2 * mask(drop, site(detgen.KIND_FF1_B), shp, wt)
    t["p0"]["u"] = orc._layer_norm(sv["h1"], sd, lp + ".2.norm")
    t["p0"]["f"], t["p0"]["dz"] = dense_front_bwd(t["p0"]["u"], src["p0"]["dg"], sd, lp + ".2.fn", drop,
                                                  site(detgen.KIND_FF1_A))
    dres = dh2 + ln_linear_bwd(sv["h1"], src["p0"]["dz"], sd, lp + ".2.norm", lp + ".2.fn.net.0.weight")
    t["dgo"] = dres * mask(drop, site(detgen.KIND_ATTN_OUT), shp, wt)
    dO = torch.matmul(src["dgo"], sd[lp + ".1.fn.to_out.0.weight"])
    t["dq"] = attn_bwd(sv["qkv"], sv["ob"], sv["lse"], dO, dtype, form)
    t["t"] = orc._layer_norm(sv["h0"], sd, lp + ".1.norm")
    t["dh0"] = ln_linear_bwd(sv["h0"], src["dq"], sd, lp + ".1.norm", lp + ".1.fn.to_qkv.weight") + dres
    return t


def branch_backward(fw, d_out, sd, m, nb, drop, dtype=F32, dev=None, form=None):
    """Every tape of modality m.  fw: {"F": [nb], "save": [nb][4]} forward tensors ([B, N, .]); d_out [B, N, DM]: the
    gradient of the branch output.  dev = None: each segment from the reference's own upstream segments (the composed
    backward).  dev = {"tape": [nb][4] dicts, "otape": [nb] dicts} (the device's): TEACHER-FORCED -- each segment from the
    DEVICE'S values of the segments upstream of it, so no error is carried from one stage into the next.
    Returns {"tape": [nb][4] (layer_backward), "otape": [nb] (out_backward), "dF0": gradient of block 0's input}."""
    DM = d_out.shape[-1]
    tapes, otapes = [None] * nb, [None] * nb
    up = d_out
    for b in reversed(range(nb)):
        devo = dev["otape"][b] if dev is not None else None
        otapes[b] = out_backward(fw["F"][b], up, sd, m, b, drop, devo)
        dF = torch.matmul((devo or otapes[b])["dz"], sd[block_prefix(m, b) + ".out_layer.net.0.weight"])   # [B, N, DM + 128]
        tapes[b] = [None] * orc.LAYERS
        later = []                                                               # (dh0, W0) of the layers above l
        for l in reversed(range(orc.LAYERS)):
            K = DM + G * l
            devt = dev["tape"][b][l] if dev is not None else None
            dfeat = dF[..., K:K + G] + sum(torch.matmul(d, w[:, K:K + G]) for d, w in later)
            tapes[b][l] = layer_backward(fw["save"][b][l], dfeat, sd, m, b, l, drop, dtype, devt, form)
            later.append(((devt or tapes[b][l])["dh0"], sd[layer_prefix(m, b, l) + ".0.weight"]))
        up = dF[..., :DM] + sum(torch.matmul(d, w[:, :DM]) for d, w in later)
    return {"tape": tapes, "otape": otapes, "dF0": up}


def _xhat(h):
    return F.layer_norm(h, (h.shape[-1],), None, None, 1e-5)


def _wg(*pairs):
    """sum over the tokens (and the operand pairs) of y[t][o] x[t][i] -> ([O, I], the same of |y| |x|)"""
    g = a = 0.0
    for y, x in pairs:
        y2, x2 = y.reshape(-1, y.shape[-1]), x.reshape(-1, x.shape[-1])
        g, a = g + torch.matmul(y2.t(), x2), a + torch.matmul(y2.abs().t(), x2.abs())
    return g, a


def _cs(terms):
    """column sum over all tokens -> (sum, sum of |terms|)"""
    t2 = terms.reshape(-1, terms.shape[-1])
    return t2.sum(0), t2.abs().sum(0)


def out_param_grads(Fb, o, bp):
    return {bp + ".out_layer.net.3.weight": _wg((o["do"], o["f"])), bp + ".out_layer.net.3.bias": _cs(o["do"]),
            bp + ".out_layer.net.0.weight": _wg((o["dz"], Fb)), bp + ".out_layer.net.0.bias": _cs(o["dz"])}


def layer_param_grads(Fk, sv, t, sd, lp):
    out = {}
    out[lp + ".0.weight"] = _wg((t["dh0"], Fk))
    out[lp + ".0.bias"] = _cs(t["dh0"])
    dt = torch.matmul(t["dq"], sd[lp + ".1.fn.to_qkv.weight"])
    out[lp + ".1.norm.weight"] = _cs(dt * _xhat(sv["h0"]))
    out[lp + ".1.norm.bias"] = _cs(dt)
    out[lp + ".1.fn.to_qkv.weight"] = _wg((t["dq"], t["t"]))
    out[lp + ".1.fn.to_out.0.weight"] = _wg((t["dgo"], sv["ob"]))
    out[lp + ".1.fn.to_out.0.bias"] = _cs(t["dgo"])
    p1, p0 = t["p1"], t["p0"]
    w1 = sd[lp + ".2.fn.net.0.weight"]
    du = torch.cat([torch.matmul(p1["dz"], w1), torch.matmul(p0["dz"], w1)], 0)      # both uses of the one ff
    xh = torch.cat([_xhat(sv["h2"]), _xhat(sv["h1"])], 0)
    out[lp + ".2.norm.weight"] = _cs(du * xh)
    out[lp + ".2.norm.bias"] = _cs(du)
    out[lp + ".2.fn.net.0.weight"] = _wg((p1["dz"], p1["u"]), (p0["dz"], p0["u"]))
    out[lp + ".2.fn.net.0.bias"] = _cs(torch.cat([p1["dz"], p0["dz"]], 0))
    out[lp + ".2.fn.net.3.weight"] = _wg((p1["dg"], p1["f"]), (p0["dg"], p0["f"]))
    out[lp + ".2.fn.net.3.bias"] = _cs(torch.cat([p1["dg"], p0["dg"]], 0))
    return out


def param_grads(fw, tp, sd, m, nb):
    """{state_dict name: (gradient, sum of |terms|)} of every block parameter of modality m, each as the contraction
    (weight matrices: tf_wgrad's TfWgradEntry table, a fixed-order sum up to 4096 tokens per modality) or the column sum
    (biases, LayerNorm parameters: colsum_atomic in the token kernels, float atomics) of the TAPE operands `tp`
    (branch_backward's result, or the device's tapes)."""
    out = {}
    for b in range(nb):
        Fb = fw["F"][b]
        out.update(out_param_grads(Fb, tp["otape"][b], block_prefix(m, b)))
        for l in range(orc.LAYERS):
            K = Fb.shape[-1] - 4 * G + G * l
            out.update(layer_param_grads(Fb[..., :K], fw["save"][b][l], tp["tape"][b][l], sd, layer_prefix(m, b, l)))
    return out


def bricks(vol):
    """[B, 1, D, H, W] (or [B, 1, H, W]) -> [B, N, 16^nd]: the patch of every token, flattened like a weight row"""
    x = vol[:, 0]
    for ax in range(1, x.dim()):
        x = x.unfold(ax, orc.PATCH, orc.PATCH)
    nd = vol.dim() - 2
    return x.reshape(x.shape[0], -1, orc.PATCH ** nd)


def embed_grads(vol, dF0, sd, m, drop):
    """patch-embedding gradients from the gradient of block 0's input (tf_dF[:, 0:DM]): the masked token gradient, summed
    over the batch (position: fixed order), over all tokens (bias: float atomics), contracted with the fp32 input bricks
    (weight: fixed order; float atomics over token chunks in the 2-D model)"""
    p = "attns.%d" % m
    dtok = dF0 * mask(drop, detgen.site_emb(m), dF0.shape, dF0.dtype)
    w = sd[p + ".patch_embeddings.weight"]
    gw, aw = _wg((dtok, bricks(vol)))
    return {p + ".position_embeddings": (dtok.sum(0, keepdim=True), dtok.abs().sum(0, keepdim=True)),
            p + ".patch_embeddings.bias": _cs(dtok),
            p + ".patch_embeddings.weight": (gw.reshape(w.shape), aw.reshape(w.shape))}


# ------------------------------------------------------------------------------------------------ readers
def state_dict_of(table, flat, dtype=torch.float64):
    """plan.table [(name, offset, numel, shape)] + the flat fp32 parameter (or gradient) buffer -> {name: tensor}"""
    flat = flat.detach().cpu()
    return {name: flat[off:off + numel].reshape(shape).to(dtype) for name, off, numel, shape in table}


def read_F(region, M, B, N, DM, nb):
    """tf_F: [nb][rows][DM + 128], row = (m B + b) N + n -> [nb][M] x [B, N, DM + 128]"""
    v = region.detach().cpu().reshape(nb, M, B, N, DM + 4 * G)
    return [[v[b, m] for m in range(M)] for b in range(nb)]


def read_save(region, M, B, N, nb, layers=orc.LAYERS):
    """tf_save: per (block, layer) rows * 232 floats, tensor-major (save_ptrs): h0 [rows][32] | qkv [96] | ob [32] | lse [8]
    | h1 [32] | h2 [32] -> [nb][layers][M] dicts of [B, N, .]"""
    rows = M * B * N
    v = region.detach().cpu().reshape(nb, layers, rows * SAVE_W)
    return [[[{k: v[b, l, rows * c0: rows * (c0 + w)].reshape(M, B, N, w)[m] for k, c0, w in SAVE_SEG}
              for m in range(M)] for l in range(layers)] for b in range(nb)]


def read_tape(region, M, B, N, nb):
    """tf_tape: per (block, layer) rows * 576 floats, SEGMENT-major: segment c of width w is [rows][w] at rows * c
    -> [nb][4][M] dicts like branch_backward's"""
    rows = M * B * N
    v = region.detach().cpu().reshape(nb, orc.LAYERS, rows * TAPE_W)

    def seg(b, l, m, c0, w):
        return v[b, l, rows * c0: rows * (c0 + w)].reshape(M, B, N, w)[m]

    def pp(b, l, m, c0):
        return {"dg": seg(b, l, m, c0, 32), "f": seg(b, l, m, c0 + 32, 64), "dz": seg(b, l, m, c0 + 96, 64),
                "u": seg(b, l, m, c0 + 160, 32)}
    return [[[{"dq": seg(b, l, m, T_DQ, 96), "t": seg(b, l, m, T_T, 32), "dh0": seg(b, l, m, T_DH0, 32),
               "p1": pp(b, l, m, T_P1), "p0": pp(b, l, m, T_P0), "dgo": seg(b, l, m, T_DGO, 32)}
              for m in range(M)] for l in range(orc.LAYERS)] for b in range(nb)]


def read_otape(region, M, B, N, DM, nb):
    """tf_otape: per block rows * (DM + 128) floats, segment-major: do [DM] | f [64] | dz [64] -> [nb][M] dicts"""
    rows = M * B * N
    v = region.detach().cpu().reshape(nb, rows * (DM + 4 * G))

    def seg(b, m, c0, w):
        return v[b, rows * c0: rows * (c0 + w)].reshape(M, B, N, w)[m]
    return [[{"do": seg(b, m, 0, DM), "f": seg(b, m, DM, 64), "dz": seg(b, m, DM + 64, 64)} for m in range(M)]
            for b in range(nb)]


def read_dF0(region, M, B, N, DM):
    """tf_dF [rows][DM + 128]: columns [0, DM) hold the gradient of block 0's input after a backward -> [M] x [B, N, DM]"""
    v = region.detach().cpu().reshape(M, B, N, DM + 4 * G)
    return [v[m, :, :, :DM] for m in range(M)]


def read_attnall(t, M, DM):
    """Runtime.read_buffer("attnall" | "g.attnall"): [B, M * DM, grid...] fp32 -> [M] x [B, N, DM]"""
    t = t.detach().cpu()
    v = t.reshape(t.shape[0], M, DM, -1)
    return [v[:, m].transpose(1, 2).contiguous() for m in range(M)]


def to_dtype(obj, dtype):
    """a nested list / dict of tensors in another float type"""
    if isinstance(obj, torch.Tensor):
        return obj.to(dtype)
    if isinstance(obj, dict):
        return {k: to_dtype(v, dtype) for k, v in obj.items()}
    return [to_dtype(v, dtype) for v in obj]
