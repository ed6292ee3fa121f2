"""tests/tf_ref.py pinned on the CPU alone, and the proof that the per-element checks of
test_gpu_transformer_rounding.py can fail.

Composition: the stage functions, composed in fp64, are oracle.hdf_oracle.transformer_branch (forward, 1e-12) and the stage
backwards + param_grads + embed_grads, composed, are autograd through that branch (every parameter of the branch, 1e-12).

Planted defects: a synthetic "kernel output" is the fp32 evaluation of a stage with ONE defect; the check the GPU module
applies to that stage (hip_util.check_rounded / check_fp32_sum / check_rounding_bias with acc = FACTOR x the fp32-vs-fp64
spread of the clean stage, per head where one head is small) must reject it and accept the clean fp32 evaluation.  For each
defect the verdict of the OLD metric (max error / max reference) at the gate that holds that code today is recorded in
OLD_GATE_PASSES: 2e-5 / 1e-4 (outputs / parameter gradients) and 1.5e-2 / 2e-3 (16-bit attention backward) of
test_gpu_transformer_ops.py, 1e-2 for a bf16 attnall, and -- for the row-statistics defect of a fused selection, which no
operator entry reaches -- the whole-model gate of test_gpu_model.py (logits at 1e-3).  The truncations, the dropped key,
the dropped token and the wrong-row rstd get past it: that is why the sharper module exists."""
import pytest
import torch
import torch.nn.functional as F

import tf_ref
from hdf_rt._lib import BF16, F16, F32
from hip_util import check_fp32_sum, check_rounded, check_rounding_bias, rel_err, rnd
from oracle import detgen
from oracle import hdf_oracle as orc
from tf_ref import acc_of

CFG = (2, 2, 16, (32, 48, 32), 8)      # two modalities, two blocks, N = 12
SEED = 77


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _sd64(cfg=CFG):
    sd = {k: v.double() for k, v in orc.det_model(*cfg).items()}
    for k in sd:                        # scores of tens in one block (the GPU module's parameter recipe)
        if ".blocks.0." in k and k.endswith("to_qkv.weight"):
            sd[k] = sd[k] * 6.0
    return sd


def _x(cfg, batch):
    x = torch.from_numpy(detgen.det_input(batch, cfg[0], cfg[3], tag="tfref")).double()
    return x + torch.arange(cfg[0], dtype=torch.float64).view(1, -1, 1, 1, 1) * 0.75 - 0.5


# ------------------------------------------------------------------------------------------------ composition
def test_the_stages_composed_are_the_oracle_branch_forward_and_backward():
    cfg, batch = CFG, 2
    nb = cfg[4] // 4
    x = _x(cfg, batch)
    for m in range(cfg[0]):
        sd = {k: v.clone().requires_grad_(k.startswith("attns.%d." % m)) for k, v in _sd64().items()}
        drop = orc.Dropper(SEED)
        vol = x[:, m:m + 1]
        ref = orc.transformer_branch(vol, sd, m, nb, drop)                    # [B, DM, grid]
        names = [k for k, v in sd.items() if v.requires_grad]
        d_out = torch.randn(ref.shape, generator=_g(3 + m), dtype=torch.float64)
        grads = dict(zip(names, torch.autograd.grad(ref, [sd[k] for k in names], d_out)))
        sdd = {k: v.detach() for k, v in sd.items()}
        with torch.no_grad():
            fw = tf_ref.branch_forward(vol, sdd, m, nb, drop)
        out = fw["out"].transpose(1, 2).reshape(ref.shape)
        assert rel_err(out, ref.detach()) < 1e-12
        # ... the pieces written out in tf_ref (attn_core, dense_parts) against the oracle's fused functions
        lp, sv = tf_ref.layer_prefix(m, 1, 2), fw["save"][1][2]
        t = orc._layer_norm(sv["h0"], sdd, lp + ".1.norm")
        att = orc._attention(t, sdd, lp + ".1.fn", drop, detgen.site_id(m, 1, 2, detgen.KIND_ATTN_OUT))
        assert rel_err(att + sv["h0"], sv["h1"]) < 1e-12
        u = orc._layer_norm(sv["h1"], sdd, lp + ".2.norm")
        _, _, g = tf_ref.dense_parts(u, sdd, lp + ".2.fn", drop, detgen.site_id(m, 1, 2, detgen.KIND_FF1_A))
        h2 = drop(g, detgen.site_id(m, 1, 2, detgen.KIND_FF1_B)) + sv["h1"]
        assert rel_err(h2, sv["h2"]) < 1e-12
        # backward: [B, DM, grid] -> [B, N, DM]
        d_tok = d_out.flatten(2).transpose(1, 2)
        tp = tf_ref.branch_backward(fw, d_tok, sdd, m, nb, drop)
        got = tf_ref.param_grads(fw, tp, sdd, m, nb)
        got.update(tf_ref.embed_grads(vol, tp["dF0"], sdd, m, drop))
        assert sorted(got) == sorted(names)
        for k in names:
            assert rel_err(got[k][0].reshape(grads[k].shape), grads[k]) < 1e-12, k
        # the teacher-forced form fed with the reference's own tapes is the composed form
        tp2 = tf_ref.branch_backward(fw, d_tok, sdd, m, nb, drop, dev=tp)
        assert rel_err(tp2["dF0"], tp["dF0"]) < 1e-13
        assert rel_err(tp2["tape"][0][1]["dh0"], tp["tape"][0][1]["dh0"]) < 1e-13


def test_the_readers_cut_the_regions_as_the_kernels_lay_them_out():
    """a region filled with its own float offsets: every named tensor must sit where transformer.h / save_ptrs put it"""
    M, B, N, DM, nb = 2, 3, 5, 64, 2
    rows, DMF = M * B * N, DM + 128
    save = tf_ref.read_save(torch.arange(nb * 4 * rows * 232, dtype=torch.float32), M, B, N, nb)
    m, b, n = 1, 2, 3
    row = (m * B + b) * N + n
    base = (1 * 4 + 2) * rows * 232
    assert float(save[1][2][m]["h0"][b, n, 7]) == base + row * 32 + 7
    assert float(save[1][2][m]["qkv"][b, n, 95]) == base + rows * 32 + row * 96 + 95
    assert float(save[1][2][m]["ob"][b, n, 0]) == base + rows * 128 + row * 32
    assert float(save[1][2][m]["lse"][b, n, 5]) == base + rows * 160 + row * 8 + 5
    assert float(save[1][2][m]["h1"][b, n, 1]) == base + rows * 168 + row * 32 + 1
    assert float(save[1][2][m]["h2"][b, n, 31]) == base + rows * 200 + row * 32 + 31
    tape = tf_ref.read_tape(torch.arange(nb * 4 * rows * 576, dtype=torch.float32), M, B, N, nb)
    base = (1 * 4 + 3) * rows * 576
    t = tape[1][3][m]
    assert float(t["dq"][b, n, 40]) == base + row * 96 + 40
    assert float(t["t"][b, n, 2]) == base + rows * 96 + row * 32 + 2
    assert float(t["dh0"][b, n, 2]) == base + rows * 128 + row * 32 + 2
    assert float(t["p1"]["dg"][b, n, 3]) == base + rows * 160 + row * 32 + 3
    assert float(t["p1"]["f"][b, n, 3]) == base + rows * 192 + row * 64 + 3
    assert float(t["p1"]["dz"][b, n, 3]) == base + rows * 256 + row * 64 + 3
    assert float(t["p1"]["u"][b, n, 3]) == base + rows * 320 + row * 32 + 3
    assert float(t["p0"]["dg"][b, n, 0]) == base + rows * 352 + row * 32
    assert float(t["p0"]["u"][b, n, 0]) == base + rows * 512 + row * 32
    assert float(t["dgo"][b, n, 9]) == base + rows * 544 + row * 32 + 9
    ot = tf_ref.read_otape(torch.arange(nb * rows * DMF, dtype=torch.float32), M, B, N, DM, nb)
    assert float(ot[1][m]["do"][b, n, 5]) == rows * DMF + row * DM + 5
    assert float(ot[1][m]["f"][b, n, 5]) == rows * DMF + rows * DM + row * 64 + 5
    assert float(ot[1][m]["dz"][b, n, 5]) == rows * DMF + rows * (DM + 64) + row * 64 + 5
    Fr = tf_ref.read_F(torch.arange(nb * rows * DMF, dtype=torch.float32), M, B, N, DM, nb)
    assert float(Fr[1][m][b, n, 100]) == rows * DMF + row * DMF + 100
    assert float(tf_ref.read_dF0(torch.arange(rows * DMF, dtype=torch.float32), M, B, N, DM)[m][b, n, 63]) == row * DMF + 63
    att = torch.arange(B * M * DM * N, dtype=torch.float32).reshape(B, M * DM, 1, N, 1)       # NCDHW, token = (d h w)
    assert float(tf_ref.read_attnall(att, M, DM)[m][b, n, 9]) == (b * M * DM + m * DM + 9) * N + n


# ------------------------------------------------------------------------------------------------ planted defects
OLD_GATE_PASSES = {}       # defect -> the old max-norm metric at its present gate lets it through


def _rejected(fn):
    with pytest.raises(AssertionError, match="outside the bound|rounding bias"):
        fn()


def _layer_case():
    """one dense layer, 1 modality, B * N = 3 * 27 = 81 rows: the sixth 16-token tile holds ONE row"""
    cfg = (1, 2, 16, (48, 48, 48), 4)
    sd64 = _sd64(cfg)
    sd32 = {k: v.float() for k, v in sd64.items()}
    drop = orc.Dropper(SEED)
    with torch.no_grad():
        fw64 = tf_ref.branch_forward(_x(cfg, 3)[:, 0:1], sd64, 0, 1, drop)
    return sd64, sd32, drop, fw64


LAYER = _layer_case()


def _ln_rows(h, g, b, eps=1e-5, steal_last=False):
    """LayerNorm(32) over the rows of h [B, N, 32] written out; steal_last: the last row of the flattened token rows takes
    the rstd of the row before it (a partial 16-token tile whose last lane group reads a neighbour's statistics)"""
    x = h.reshape(-1, h.shape[-1])
    mean = x.mean(-1, keepdim=True)
    rstd = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
    if steal_last:
        assert x.shape[0] % 16 != 0
        rstd = rstd.clone()
        rstd[-1] = rstd[-2]
    return ((x - mean) * rstd * g + b).reshape(h.shape)


def test_a_dropout_mask_of_the_neighbouring_site_is_rejected():
    sd64, sd32, drop, fw = LAYER
    lp, sv = tf_ref.layer_prefix(0, 0, 2), fw["save"][0][2]
    site = detgen.site_id(0, 0, 2, detgen.KIND_ATTN_OUT)
    ref64 = tf_ref.post_h1(sv["ob"], sv["h0"], sd64, lp, drop, site)
    ref32 = tf_ref.post_h1(sv["ob"].float(), sv["h0"].float(), sd32, lp, drop, site)
    acc = acc_of("h1", ref32, ref64)
    assert check_rounded(ref32, ref64, F32, acc) <= 1.0
    bad = tf_ref.post_h1(sv["ob"].float(), sv["h0"].float(), sd32, lp, drop, site + 1)
    _rejected(lambda: check_rounded(bad, ref64, F32, acc))
    OLD_GATE_PASSES["dropout_site"] = rel_err(bad, ref32) < 2e-5


@pytest.mark.parametrize("defect", ["eps_missing", "rstd_of_the_row_before"])
def test_layernorm_defects_are_rejected(defect):
    sd64, sd32, drop, fw = LAYER
    lp = tf_ref.layer_prefix(0, 0, 1)
    Fk = fw["F"][0][..., :64 + 32]
    h0, t64, q64 = tf_ref.pre(Fk, sd64, lp)
    _, t32, q32 = tf_ref.pre(Fk.float(), sd32, lp)
    g, b = sd32[lp + ".1.norm.weight"], sd32[lp + ".1.norm.bias"]
    assert rel_err(_ln_rows(h0.float(), g, b), t32) < 1e-6            # the written-out form is the LayerNorm
    bad_t = _ln_rows(h0.float(), g, b, eps=0.0) if defect == "eps_missing" else _ln_rows(h0.float(), g, b, steal_last=True)
    bad_q = F.linear(bad_t, sd32[lp + ".1.fn.to_qkv.weight"])
    for name, ref32, ref64, bad in (("t", t32, t64, bad_t), ("qkv", q32, q64, bad_q)):
        acc = acc_of(name, ref32, ref64)
        assert check_rounded(ref32, ref64, F32, acc) <= 1.0
        _rejected(lambda: check_rounded(bad, ref64, F32, acc))
    OLD_GATE_PASSES[defect] = rel_err(bad_q, q32) < 2e-5
    if defect == "rstd_of_the_row_before":
        # No operator entry runs the fused selections: what holds them today is the whole-model gate (logits at 1e-3 of the
        # maximum, test_gpu_model.py) on the closed-form weights and inputs of oracle/detgen.py, whose tokens are nearly
        # alike -- neighbouring rows have nearly the same rstd.  The same defect inside the oracle's model, in LayerNorm 1 of
        # one layer, eval mode, at the N = 27 / batch 3 geometry: measured 7.3e-4, 4.6e-4, 3.9e-4, 2.6e-4 on the four
        # outputs.  (Where it sits matters: in LayerNorm 2 of layer 3, or in train mode, the same gate sees 1e-2 .. 5e-2.)
        cfg = (1, 2, 16, (48, 48, 48), 4)
        sdm = orc.det_model(*cfg)
        x = torch.from_numpy(detgen.det_input(3, cfg[0], cfg[3], tag="smoke"))
        clean = orc.forward(x, sdm, None)
        orig = orc._layer_norm

        def stolen(xx, sd, p):
            if p == lp + ".1.norm":
                return _ln_rows(xx, sd[p + ".weight"], sd[p + ".bias"], steal_last=True)
            return orig(xx, sd, p)
        orc._layer_norm = stolen
        try:
            bad = orc.forward(x, sdm, None)
        finally:
            orc._layer_norm = orig
        errs = [rel_err(a, c) for a, c in zip(bad, clean)]
        assert min(errs) > 1e-5                                         # the defect did reach every output
        OLD_GATE_PASSES["rstd_of_the_row_before.model_gate"] = max(errs) < 1e-3
        print("whole-model effect of the wrong-row rstd: %s" % ["%.2e" % e for e in errs])


def test_tanh_gelu_is_rejected():
    sd64, sd32, drop, fw = LAYER
    lp, sv = tf_ref.layer_prefix(0, 0, 0), fw["save"][0][0]
    sa, sb = detgen.site_id(0, 0, 0, detgen.KIND_FF1_A), detgen.site_id(0, 0, 0, detgen.KIND_FF1_B)
    ref64 = tf_ref.ff(sv["h1"], sd64, lp, drop, sa, sb) + sv["h1"]
    h32 = sv["h1"].float()
    ref32 = tf_ref.ff(h32, sd32, lp, drop, sa, sb) + h32
    acc = acc_of("h2", ref32, ref64)
    assert check_rounded(ref32, ref64, F32, acc) <= 1.0
    u = orc._layer_norm(h32, sd32, lp + ".2.norm")
    f = drop(F.gelu(F.linear(u, sd32[lp + ".2.fn.net.0.weight"], sd32[lp + ".2.fn.net.0.bias"]), approximate="tanh"), sa)
    bad = drop(F.linear(f, sd32[lp + ".2.fn.net.3.weight"], sd32[lp + ".2.fn.net.3.bias"]), sb) + h32
    _rejected(lambda: check_rounded(bad, ref64, F32, acc))
    OLD_GATE_PASSES["tanh_gelu"] = rel_err(bad, ref32) < 2e-5


def _per_head(stage, got, ref32, ref64, width, check=check_rounded, alt64=None, extra=None):
    """the check per head (tf_ref.group_accs): a head a thousand times smaller than the others is held as tightly as they"""
    worst = 0.0
    for s, acc in tf_ref.group_accs(stage, ref32, ref64, width, alt64):
        if extra is not None:
            acc = acc + extra[..., s]
        what = "%s columns %s" % (stage, s)
        worst = max(worst, check(got[..., s], ref64[..., s], F32, acc, what) if check is check_rounded
                    else check(got[..., s], ref64[..., s], acc, what))
    return worst


def test_a_key_left_out_of_one_softmax_row_and_a_base_2_lse_are_rejected():
    nseq, N = 3, 64
    qkv, _ = tf_ref.attn_inputs(nseq, N, 5, peaked=False)
    ob64, lse64 = tf_ref.attn_core(qkv.double())
    ob32, lse32 = tf_ref.attn_core(qkv)
    assert _per_head("ob", ob32, ob32, ob64, 4) <= 1.0
    # the last query of the last sequence never sees the last key, in the small head
    q, k, v = [tf_ref.heads(t) for t in qkv.split(32, dim=-1)]
    s = torch.matmul(q, k.transpose(-1, -2)) * 0.5
    s[nseq - 1, 7, N - 1, N - 1] = float("-inf")
    bad = tf_ref.merge(torch.matmul(torch.softmax(s, dim=-1), v))
    _rejected(lambda: _per_head("ob", bad, ob32, ob64, 4))
    OLD_GATE_PASSES["dropped_key"] = rel_err(bad, ob32) < 2e-5
    acc = acc_of("lse", lse32, lse64)
    assert check_rounded(lse32, lse64, F32, acc) <= 1.0
    _rejected(lambda: check_rounded(lse32 / 0.6931471805599453, lse64, F32, acc))
    OLD_GATE_PASSES["lse_base2"] = rel_err(lse32 / 0.6931471805599453, lse32) < 2e-5


def test_a_token_left_out_and_a_tape_of_the_layer_below_are_rejected_in_a_weight_gradient():
    """to_out.weight = sum over the tokens of dgo[t][o] ob[t][i] at the benchmark's 2 x 512 tokens per modality; head 7 of
    ob is the small one"""
    T = 1024
    g = _g(11)
    dgo, dgo_below = torch.randn(T, 32, generator=g), torch.randn(T, 32, generator=g)
    ob = torch.randn(T, 32, generator=g)
    ob[:, 28:] *= 1e-3
    ref64 = tf_ref._wg((dgo.double(), ob.double()))[0]
    ref32 = tf_ref._wg((dgo, ob))[0]
    assert _per_head("wgrad", ref32, ref32, ref64, 4, check=check_fp32_sum) <= 1.0
    dropped = dgo.clone()
    dropped[-1, 16:] = 0                      # the last token never reaches the second 16-row tile, seen in head 7's columns
    bad = tf_ref._wg((dropped, ob))[0]
    bad[:, :28] = ref32[:, :28]
    _rejected(lambda: _per_head("wgrad", bad, ref32, ref64, 4, check=check_fp32_sum))
    OLD_GATE_PASSES["dropped_token"] = rel_err(bad, ref32) < 1e-4
    below = tf_ref._wg((dgo_below, ob))[0]
    _rejected(lambda: _per_head("wgrad", below, ref32, ref64, 4, check=check_fp32_sum))
    OLD_GATE_PASSES["tape_of_layer_below"] = rel_err(below, ref32) < 1e-4


def _trunc_round(t, dtype):
    if dtype == F32:
        return t
    mask = ~0xFFFF if dtype == BF16 else ~0x1FFF
    return (t.float().contiguous().view(torch.int32) & mask).view(torch.float32).to(t.dtype)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_truncated_16_bit_operands_of_the_attention_backward_are_rejected(dtype):
    nseq, N = 2, 64
    qkv, d_ob = tf_ref.attn_inputs(nseq, N, 21, peaked=False)
    ob, lse = tf_ref.attn_core(qkv)
    ref64 = tf_ref.attn_bwd(qkv.double(), ob.double(), lse.double(), d_ob.double(), dtype)
    alt64 = tf_ref.attn_bwd(qkv.double(), ob.double(), lse.double(), d_ob.double(), dtype, form=torch.float32)
    ref32 = tf_ref.attn_bwd(qkv, ob, lse, d_ob, dtype)
    amb = tf_ref.attn_bwd_ambiguity(qkv, ob, lse, d_ob, dtype, tf_ref.FACTOR.get("tape.dq", 4.0))
    floor = tf_ref.attn_bwd_ambiguity(qkv, ob, lse, d_ob, F32)
    share = float((amb > floor).double().mean())      # elements with an operand on a rounding tie
    assert share > 0.0
    assert _per_head("tape.dq", ref32, ref32, ref64, 4, alt64=alt64, extra=amb) <= 1.0
    orig = tf_ref.lp_round
    tf_ref.lp_round = _trunc_round
    try:
        bad = tf_ref.attn_bwd(qkv, ob, lse, d_ob, dtype)
    finally:
        tf_ref.lp_round = orig
    _rejected(lambda: _per_head("tape.dq", bad, ref32, ref64, 4, alt64=alt64, extra=amb))
    gate = {BF16: 1.5e-2, F16: 2e-3}[dtype]
    OLD_GATE_PASSES["truncated_operands.%d" % dtype] = all(
        rel_err(bad[..., 32 * i:32 * i + 32], ref32[..., 32 * i:32 * i + 32]) < gate for i in range(3))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_a_truncated_attnall_store_is_rejected(dtype):
    sd64, sd32, drop, fw = LAYER
    bp = tf_ref.block_prefix(0, 0)
    Fb = torch.cat([fw["F"][0]] * 8, 0)       # 648 tokens x 64 columns: enough elements for the bias statistic
    drop = orc.Dropper(None)
    ref64 = tf_ref.block_out(Fb, sd64, bp, drop, 0, 0)
    ref32 = tf_ref.block_out(Fb.float(), sd32, bp, drop, 0, 0)
    acc = acc_of("attnall", ref32, ref64)
    good = rnd(ref32, dtype)
    assert check_rounded(good, ref64, dtype, acc) <= 1.0
    check_rounding_bias(good, ref64, dtype)
    bad = _trunc_round(ref32, dtype)
    _rejected(lambda: check_rounded(bad, ref64, dtype, acc))
    _rejected(lambda: check_rounding_bias(bad, ref64, dtype))
    OLD_GATE_PASSES["truncated_attnall.%d" % dtype] = rel_err(bad, ref32) < 1e-2


def test_the_old_metric_lets_the_quiet_defects_through():
    """the verdicts the tests above recorded (run here for whichever of them was deselected)"""
    fill = [(test_a_dropout_mask_of_the_neighbouring_site_is_rejected, (), "dropout_site"),
            (test_layernorm_defects_are_rejected, ("eps_missing",), "eps_missing"),
            (test_layernorm_defects_are_rejected, ("rstd_of_the_row_before",), "rstd_of_the_row_before"),
            (test_tanh_gelu_is_rejected, (), "tanh_gelu"),
            (test_a_key_left_out_of_one_softmax_row_and_a_base_2_lse_are_rejected, (), "dropped_key"),
            (test_a_token_left_out_and_a_tape_of_the_layer_below_are_rejected_in_a_weight_gradient, (), "dropped_token"),
            (test_truncated_16_bit_operands_of_the_attention_backward_are_rejected, (BF16,), "truncated_operands.1"),
            (test_truncated_16_bit_operands_of_the_attention_backward_are_rejected, (F16,), "truncated_operands.2"),
            (test_a_truncated_attnall_store_is_rejected, (BF16,), "truncated_attnall.1"),
            (test_a_truncated_attnall_store_is_rejected, (F16,), "truncated_attnall.2")]
    for fn, args, key in fill:
        if key not in OLD_GATE_PASSES:
            fn(*args)
    need = ["dropout_site", "eps_missing", "rstd_of_the_row_before", "rstd_of_the_row_before.model_gate", "tanh_gelu",
            "dropped_key", "lse_base2", "dropped_token", "tape_of_layer_below", "truncated_operands.1",
            "truncated_operands.2", "truncated_attnall.1", "truncated_attnall.2"]
    assert sorted(OLD_GATE_PASSES) == sorted(need), sorted(OLD_GATE_PASSES)
    print("old max-norm gate lets through: %s" % {k: bool(v) for k, v in sorted(OLD_GATE_PASSES.items())})
    for k in ("truncated_operands.1", "truncated_operands.2", "truncated_attnall.1", "truncated_attnall.2", "dropped_key",
              "dropped_token", "rstd_of_the_row_before.model_gate"):
        assert OLD_GATE_PASSES[k], k
    for k in ("dropout_site", "lse_base2", "tape_of_layer_below"):      # loud defects: any metric sees them
        assert not OLD_GATE_PASSES[k], k
