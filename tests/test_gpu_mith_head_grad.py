"""GPU: MITH's hash head in training mode (xmh_mith_grad.hip behind torch.autograd in MITHHashLayer.encode_img_train /
encode_txt_train) against the goldens of the reference's own HashLayer and against the float64 restatement of
tests/mith_head_grad_cases.py; the exact zeros of masked tokens and empty concepts, absent upstream gradients, the shared
GlobalConceptLearning, frozen parameters, the accumulate flag, reproducibility, bit identity of the hashes with the eval path and of
xmh_lta_aggregate with its earlier kernel, no host synchronisation, autograd's guards, and three BertAdam steps of the heads over a
frozen backbone against the float64 trajectory.

Tolerances: the rule of tests/test_gpu_block_grad.py.  Per tensor e = max|got - fp64| / max|fp64| (absolute for tensors that are
identically zero); the port must stay within TOL_FACTOR = 4 times the pooled e_ref of that tensor kind from the golden file,
TOL_FACTOR + 1 against the thinned fp32 golden itself; on shapes outside the pool 4 * max(pool, that case's own e_ref), measured here
from the restatement's fp32 run on the CPU.

Selection ties.  The LTA keep-set is discontinuous (score > 0, the top_k-th rank), so the float64 restatement is evaluated with the
keep-set the forward stored (A != 0), never the other way round; before that the stored set must differ from the float64 set in at
most 0.5 % of the case's [B, L, K] entries, each of them within 8 eps |score| of its threshold in float64.

Every figure is printed before the first assertion."""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import mith_head_grad_cases as MC

pytestmark = pytest.mark.gpu

TOL_FACTOR = 4.0
EPS = float(np.finfo(np.float32).eps)


# ---- the head under test ---------------------------------------------------------------------------------------------------------
def _head(sd, D, layers, R, K, top_k):
    """MITHHashLayer on the device with the case's parameters in BOTH modalities' places"""
    from xmh.models.mith import MITHHashLayer
    h = MITHHashLayer(D, K, 0.0, layers, "gelu", top_k, R)
    with torch.no_grad():
        for i in range(R):
            ln, mlp = h.gcl_i.mlp.lns[i], h.gcl_i.mlp.mlps[i]
            for p, f in zip((ln.weight, ln.bias, mlp[0].weight, mlp[0].bias, mlp[3].weight, mlp[3].bias), MC.MLP_FIELDS):
                p.copy_(torch.tensor(sd["mlp%d.%s" % (i, f)]))
        h.gcl_i.common_concept_embedding.weight.copy_(torch.tensor(sd["concept"]))
        for lct, proj in ((h.lct_i, h.img_concept_proj), (h.lct_t, h.txt_concept_proj)):
            lct.transformer.load_state_dict({k[len("blk."):]: torch.tensor(v) for k, v in sd.items() if k.startswith("blk.")}, strict=True)
            for k, fc in enumerate(lct.hashing.fc_list):
                fc.weight.copy_(torch.tensor(sd["hash_w"][k:k + 1]))
                fc.bias.copy_(torch.tensor(sd["hash_b"][k:k + 1]))
            proj.weight.copy_(torch.tensor(sd["proj_w"]))
            proj.bias.copy_(torch.tensor(sd["proj_b"]))
    return h.cuda()


def _parts(h, mod):
    return (h.gcl_i, h.lct_i, h.img_concept_proj) if mod == "img" else (h.gcl_t, h.lct_t, h.txt_concept_proj)


def _encode(h, mod, ct, tt, mask):
    m = None if mask is None else torch.tensor(mask).cuda()
    return h.encode_img_train(ct, tt) if mod == "img" else h.encode_txt_train(ct, tt, m)


def _grads(h, mod, R, layers):
    """the parameters' .grad under the restatement's tensor names (None where there is none)"""
    from xmh.models import clip_train as CT
    gcl, lct, proj = _parts(h, mod)
    g = lambda p: None if p.grad is None else p.grad.detach().cpu().numpy()      # noqa: E731
    out = {}
    for i in range(R):
        ln, mlp = gcl.mlp.lns[i], gcl.mlp.mlps[i]
        for p, f in zip((ln.weight, ln.bias, mlp[0].weight, mlp[0].bias, mlp[3].weight, mlp[3].bias), MC.MLP_FIELDS):
            out["g_mlp%d_%s" % (i, f)] = g(p)
    out["g_concept"] = g(gcl.common_concept_embedding.weight)
    for i, blk in enumerate(lct.transformer.resblocks):
        for (kind, _), p in zip(MC.BC.PARAMS, [CT._get[path](blk) for _, path in CT.BLOCK]):
            out["g_l%d_%s" % (i, kind)] = g(p)
    ws, bs = [g(fc.weight) for fc in lct.hashing.fc_list], [g(fc.bias) for fc in lct.hashing.fc_list]
    out["g_hash_w"] = None if any(w is None for w in ws) else np.concatenate(ws, 0)
    out["g_hash_b"] = None if any(b is None for b in bs) else np.concatenate(bs, 0)
    out["g_proj_w"], out["g_proj_b"] = g(proj.weight), g(proj.bias)
    return out


def _step(h, mod, cls, tok, mask, ups, R, layers, in_grad=True):
    """forward + backward of sum_i (output_i . up_i).sum() -> the restatement's dict"""
    ct, tt = torch.tensor(cls).cuda().requires_grad_(in_grad), torch.tensor(tok).cuda().requires_grad_(in_grad)
    outs = _encode(h, mod, ct, tt, mask)
    B, K = outs[1].shape
    assert all(o.requires_grad and o.dtype == torch.float32 and o.is_cuda for o in outs)
    assert [tuple(o.shape) for o in outs] == [tuple(cls.shape), (B, K), (B, K), (K, B, cls.shape[1])]
    sum((o * torch.tensor(u).cuda()).sum() for o, u in zip(outs, ups) if u is not None).backward()
    out = {n: o.detach().cpu().numpy() for n, o in zip(MC.OUTPUTS, outs)}
    out["g_cls"] = None if ct.grad is None else ct.grad.cpu().numpy()
    out["g_tokens"] = None if tt.grad is None else tt.grad.cpu().numpy()
    out.update(_grads(h, mod, R, layers))
    return out


def _stored_attention(h, mod, cls, tok, mask):
    """A [B, K, L] as the forward stores it, and the scores' keep-set [L, B, K] it implies"""
    from xmh.models import mith as M
    gcl, lct, proj = _parts(h, mod)
    m = None if mask is None else torch.tensor(mask).cuda().to(torch.uint8)
    tokens = torch.tensor(tok).cuda().permute(1, 0, 2)
    outs, kept = M._head_forward(gcl, lct, m, torch.tensor(cls).cuda(), tokens, M.head_params(gcl, lct, proj))
    A = M.saved_attention(kept[3], kept[4]).cpu()
    return A.numpy(), (A != 0).permute(2, 0, 1).numpy(), outs


_refs = {}


def _reference(key, sd, cls, tok, mask, ups, heads, top_k, keep, with_f32=False):
    """the float64 restatement under the stored keep-set (and its fp32 run where asked for), computed once per key and shared"""
    if key not in _refs:
        r64 = MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float64, keep=keep)
        pool = MC.erefs(MC.run_restatement(sd, cls, tok, mask, ups, heads, top_k, torch.float32, keep=keep), r64)[1] if with_f32 else {}
        _refs[key] = (r64, pool)
    return _refs[key]


def _check_selection(what, sd, cls, tok, mask, heads, top_k, keep):
    """the stored keep-set against the float64 one: at most 0.5 % of the entries differ, each within 8 eps |score| of its threshold"""
    s64 = []
    r = MC.run_restatement(sd, cls, tok, mask, (None, None, np.zeros((keep.shape[1], keep.shape[2]), np.float32), None), heads, top_k,
                           torch.float64, scores_out=s64)
    k64, margin = MC.selection(s64[0], mask, top_k)
    assert np.array_equal(k64.numpy(), r["keep"])
    diff = np.argwhere(k64.numpy() != keep)
    worst = max([float(margin[tuple(i)] / (8 * EPS * abs(float(s64[0][tuple(i)])))) for i in diff], default=0.0)
    print(what, "keep-set: %d of %d entries kept, %d differ from the float64 set, largest margin / (8 eps |score|) %.2f"
          % (int(keep.sum()), keep.size, len(diff), worst))
    assert len(diff) <= 0.005 * keep.size, (what, len(diff))
    assert worst <= 1.0, (what, worst)
    return k64.numpy()


def _check(got, R, what, own=None, kinds=None):
    """every figure is printed before the first assertion"""
    rows = []
    for k in R:
        kind = MC.kind_of(k)
        if k == "keep" or got.get(k) is None or (kinds is not None and kind not in kinds):
            continue
        tol = TOL_FACTOR * max(MC.pool_eref(kind), (own or {}).get(kind, 0.0))
        rows.append((k, MC.rel_err(got[k], R[k]), tol))
    print(what, " ".join("%s %.2e/%.2e" % r for r in rows))
    worst = {}
    for k, e, tol in rows:
        kind = MC.kind_of(k)
        worst[kind] = max(worst.get(kind, 0.0), e / (tol / TOL_FACTOR))
    print(what, "e_port / e_ref per kind:", " ".join("%s %.2f" % (k, v) for k, v in worst.items()))
    for k, e, tol in rows:
        assert got[k].shape == R[k].shape and np.isfinite(got[k]).all(), (what, k)
        assert e <= tol, (what, k, e, tol)
    return rows


# 1 goldens -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", list(MC.CASES))
def test_every_output_and_gradient_matches_the_reference(case):
    G = MC.golden()
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    assert MC.inputs_checksum(sd, cls, tok, mask, ups) == float(G[case + "__checksum"])
    h = _head(sd, D, layers, R, K, top_k)
    A, keep, _ = _stored_attention(h, mod, cls, tok, mask)
    k64 = _check_selection(case, sd, cls, tok, mask, heads, top_k, keep)
    Rf, _ = _reference(case, sd, cls, tok, mask, ups, heads, top_k, keep)
    got = _step(h, mod, cls, tok, mask, ups, R, layers)
    assert sorted(got) == sorted(k for k in Rf if k != "keep") and all(v is not None for v in got.values())
    rows = []
    if np.array_equal(keep, k64):                                  # the golden belongs to the reference's keep-set
        for k in got:
            err = np.abs(MC.thin(got[k]).astype(np.float64) - G["%s__%s" % (case, k)].astype(np.float64)).max() / (np.abs(Rf[k]).max() or 1.0)
            rows.append((k, err, (TOL_FACTOR + 1) * MC.pool_eref(MC.kind_of(k))))
        print(case, "against the fp32 golden:", " ".join("%s %.2e/%.2e" % r for r in rows))
    _check(got, Rf, case)
    for k, err, tol in rows:
        assert err <= tol, (case, "golden", k, err, tol)
    # the exact zeros
    rows_sum = A.sum(axis=2)                                       # [B, K]: 1 where a concept has tokens, 0 where it has none
    assert np.all((np.abs(rows_sum - 1) < 1e-5) | (rows_sum == 0))
    if case in MC.EMPTY_CONCEPT_CASES:
        empty = ~keep.any(axis=0)                                  # [B, K]
        assert empty.any() and not A[empty].any()                  # the NaN -> 0 route: that row of A exactly zero
    if mask is not None:
        assert not A.transpose(0, 2, 1)[mask].any()                # [B, L, K] at the masked tokens
        assert not got["g_tokens"].transpose(1, 0, 2)[mask].any()  # masked tokens get exactly zero
        dropped = ~keep.any(axis=2).T                              # [B, L]: tokens no concept kept
        assert not got["g_tokens"].transpose(1, 0, 2)[dropped].any()
    if mk == "pad_all":
        assert mask[1].all() and not A[1].any() and not got["g_tokens"][:, 1].any()      # M = pe for that sample, and nothing flows back


# 2 other shapes ----------------------------------------------------------------------------------------------------------------
SHAPES = [(512, 8, 2, 2, 64, 8, 49, 2, "img", None),          # the workload's image side, two samples
          (512, 8, 2, 2, 16, 8, 32, 2, "txt", "pad"),         # its text side at 16 bits
          (64, 1, 1, 1, 33, 33, 65, 5, "txt", "pad")]         # top_k = K, L behind one 64-token group, B = 5


def _shape_inputs(shape):
    D, heads, layers, R, K, top_k, L, B, mod, mk = shape
    seed = 7000 + D + 7 * L + K + B
    cls, tok, ups = MC.draw_batch(seed, B, L, D, K)
    return MC.draw_params(seed, D, layers, R, K), cls, tok, MC.draw_mask(seed, B, L, mk), ups


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "d%d_h%d_n%d_r%d_k%d_top%d_l%d_b%d_%s" % s[:9])
def test_against_the_restatement_on_other_shapes(shape):
    D, heads, layers, R, K, top_k, L, B, mod, mk = shape
    sd, cls, tok, mask, ups = _shape_inputs(shape)
    h = _head(sd, D, layers, R, K, top_k)
    _, keep, _ = _stored_attention(h, mod, cls, tok, mask)
    _check_selection(str(shape), sd, cls, tok, mask, heads, top_k, keep)
    Rf, own = _reference(shape, sd, cls, tok, mask, ups, heads, top_k, keep, with_f32=True)
    print("e_ref of this case:", " ".join("%s %.2e" % kv for kv in sorted(own.items())))
    got = _step(h, mod, cls, tok, mask, ups, R, layers)
    _check(got, Rf, str(shape), own=own)


# 3 absent upstream gradients, the shared gcl -------------------------------------------------------------------------------------
def test_absent_upstreams_give_exact_zeros():
    """only tokens_hash enters the objective (as in generate_hash): what the other paths alone feed is exactly zero"""
    case = "d128_k16_top8_l7_r2_txt"
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    full = _step(_head(sd, D, layers, R, K, top_k), mod, cls, tok, mask, ups, R, layers)
    only = (None, None, ups[2], None)
    got = _step(_head(sd, D, layers, R, K, top_k), mod, cls, tok, mask, only, R, layers)
    for k, v in got.items():
        if k in ("g_proj_w", "g_proj_b", "g_concept", "g_cls") or k.startswith("g_mlp"):
            assert v is not None and v.shape == full[k].shape and not v.any(), k
    assert got["g_hash_w"].any() and got["g_hash_b"].any() and got["g_tokens"].any() and got["g_l0_qkv_w"].any()
    _, keep, _ = _stored_attention(_head(sd, D, layers, R, K, top_k), mod, cls, tok, mask)
    Rf, _ = _reference((case, "only tokens_hash"), sd, cls, tok, mask, only, heads, top_k, keep)
    _check(got, Rf, "only tokens_hash", kinds=("g_hash_w", "g_hash_b", "g_tokens") + tuple("g_blk_" + k for k, _ in MC.BC.PARAMS))
    # the other way round: no token path
    got = _step(_head(sd, D, layers, R, K, top_k), mod, cls, tok, mask, (ups[0], ups[1], None, None), R, layers)
    for k, v in got.items():
        if k in ("g_proj_w", "g_proj_b", "g_hash_w", "g_hash_b", "g_tokens") or (k.startswith("g_l") and k[3].isdigit()):
            assert v is not None and not v.any(), k
    Rf, _ = _reference((case, "cls path"), sd, cls, tok, mask, (ups[0], ups[1], None, None), heads, top_k, keep)
    _check(got, Rf, "cls path only", kinds=("g_concept", "g_cls") + tuple("g_mlp_" + f for f in MC.MLP_FIELDS))


def test_gcl_grad_is_the_sum_of_both_modalities():
    case = "d128_k16_top8_l7_r2_txt"
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    cls2, tok2, ups2 = MC.draw_batch(99, B, L + 2, D, K)
    txt = _step(_head(sd, D, layers, R, K, top_k), "txt", cls, tok, mask, ups, R, layers)
    img = _step(_head(sd, D, layers, R, K, top_k), "img", cls2, tok2, None, ups2, R, layers)
    h = _head(sd, D, layers, R, K, top_k)
    assert h.gcl_i is h.gcl_t
    oi = h.encode_img_train(torch.tensor(cls2).cuda(), torch.tensor(tok2).cuda())
    ot = h.encode_txt_train(torch.tensor(cls).cuda(), torch.tensor(tok).cuda(), torch.tensor(mask).cuda())
    (sum((o * torch.tensor(u).cuda()).sum() for o, u in zip(oi, ups2)) + sum((o * torch.tensor(u).cuda()).sum() for o, u in zip(ot, ups))).backward()
    both_i, both_t = _grads(h, "img", R, layers), _grads(h, "txt", R, layers)
    for k in both_i:
        if k == "g_concept" or k.startswith("g_mlp"):
            assert np.array_equal(both_i[k], img[k] + txt[k]), k       # one addition of two fp32 tensors: the same in either order
        else:
            assert np.array_equal(both_i[k], img[k]) and np.array_equal(both_t[k], txt[k]), k


# 4 frozen parameters, accumulate, reproducibility --------------------------------------------------------------------------------
def test_frozen_parameters_get_none_and_the_others_keep_their_bits():
    case = "k20_top8_l50_r1_txt_allmasked"
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    full = _step(_head(sd, D, layers, R, K, top_k), mod, cls, tok, mask, ups, R, layers)
    again = _step(_head(sd, D, layers, R, K, top_k), mod, cls, tok, mask, ups, R, layers)
    assert all(np.array_equal(full[k], again[k]) for k in full)                      # two runs agree to the bit
    h = _head(sd, D, layers, R, K, top_k)
    frozen = {"gcl_i.mlp.lns.0.weight", "gcl_i.mlp.mlps.0.3.weight", "lct_t.transformer.resblocks.0.attn.in_proj_weight",
              "lct_t.transformer.resblocks.1.ln_2.bias", "txt_concept_proj.weight", "gcl_i.common_concept_embedding.weight"}
    frozen |= {"lct_t.hashing.fc_list.%d.bias" % k for k in range(K)}
    for n, p in h.named_parameters():
        p.requires_grad_(n not in frozen)
    got = _step(h, mod, cls, tok, mask, ups, R, layers, in_grad=False)
    want_none = {"g_mlp0_ln_w", "g_mlp0_fc2_w", "g_l0_qkv_w", "g_l1_ln2_b", "g_proj_w", "g_concept", "g_hash_b", "g_cls", "g_tokens"}
    for k, v in got.items():
        assert (v is None) == (k in want_none), k
        if v is not None:
            assert np.array_equal(v, full[k]), k
    for p in h.parameters():                                                         # the whole head frozen, the inputs not: dx alone
        p.requires_grad_(False)
        p.grad = None
    got = _step(h, mod, cls, tok, mask, ups, R, layers)
    assert all(v is None for k, v in got.items() if k.startswith("g_") and k not in ("g_cls", "g_tokens"))
    assert np.array_equal(got["g_cls"], full["g_cls"]) and np.array_equal(got["g_tokens"], full["g_tokens"])


def test_accumulate_adds_at_the_c_level_and_argument_errors():
    from xmh import _lib
    from xmh._lib import current_stream, lib, ptr
    from xmh.models import clip_train as CT
    from xmh.models import mith as M
    case = "k8_top8_l7_r2_img"
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    h = _head(sd, D, layers, R, K, top_k)
    gcl, lct, proj = _parts(h, mod)
    params = M.head_params(gcl, lct, proj)
    outs, (desc, keep, cls_c, buf, geom, nbytes) = M._head_forward(gcl, lct, None, torch.tensor(cls).cuda(), torch.tensor(tok).cuda().permute(1, 0, 2), params)
    gg = [torch.tensor(u).cuda() for u in ups]
    pm, ci, pb, hw, hb, pw, pbias = M._split(list(range(len(params))), R, layers, K)

    def run(accumulate, init=None, saved_bytes=None, ws_bytes=None):
        bufs = {}
        mk_ = lambda name, shape: bufs.setdefault(name, torch.full(shape, float("nan"), device="cuda") if init is None else init[name].clone())      # noqa: E731
        gp = [None] * len(params)
        for i in pm + [ci] + pb + [pw, pbias]:
            gp[i] = mk_("p%d" % i, tuple(params[i].shape))
        d_hw, d_hb, d_cls, d_tok = mk_("hash_w", (K, D)), mk_("hash_b", (K,)), mk_("d_cls", (B, D)), mk_("d_tokens", (B, L, D))
        mg = (_lib.MithMlpGrads * max(R, 1))()
        for i in range(R):
            mg[i] = _lib.MithMlpGrads(*[gp[j].data_ptr() for j in pm[6 * i:6 * i + 6]])
        bg = CT.block_grads([gp[j] for j in pb])
        grads = _lib.MithGrads(mg, gp[ci].data_ptr(), bg, d_hw.data_ptr(), d_hb.data_ptr(), gp[pw].data_ptr(), gp[pbias].data_ptr(), d_cls.data_ptr(),
                               d_tok.data_ptr())
        ws = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        rc = lib.xmh_mith_train_backward(ctypes.byref(desc), ptr(cls_c), B, L, *(ptr(g) for g in gg), ptr(buf),
                                         buf.numel() * 4 if saved_bytes is None else saved_bytes, ctypes.byref(grads), accumulate, ptr(ws),
                                         nbytes if ws_bytes is None else ws_bytes, current_stream())
        return bufs, rc
    a, rc = run(0)
    assert rc == 0 and all(bool(torch.isfinite(t).all()) for t in a.values())
    b, rc = run(0)
    assert rc == 0 and all(torch.equal(a[k], b[k]) for k in a)
    g = torch.Generator(device="cuda").manual_seed(3)
    g0 = {k: torch.randn(t.shape, device="cuda", generator=g) for k, t in a.items()}
    acc, rc = run(1, init=g0)
    assert rc == 0
    for k in a:
        want = a[k] if k in ("d_cls", "d_tokens") else g0[k] + a[k]                   # activation gradients: written, never added to
        assert torch.equal(acc[k], want), k
    assert run(0, saved_bytes=buf.numel() * 4 - 4)[1] == -12 and b"saved" in lib.xmh_last_error()
    assert run(0, ws_bytes=nbytes - 1)[1] == -12 and b"workspace" in lib.xmh_last_error()
    # the autograd path returns the same bits
    s = _step(_head(sd, D, layers, R, K, top_k), mod, cls, tok, mask, ups, R, layers)
    assert np.array_equal(s["g_cls"], a["d_cls"].cpu().numpy()) and np.array_equal(s["g_tokens"], a["d_tokens"].permute(1, 0, 2).cpu().numpy())
    assert np.array_equal(s["g_hash_w"], a["hash_w"].cpu().numpy()) and np.array_equal(s["g_concept"], a["p%d" % ci].cpu().numpy())


# 5 forward -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["k20_top8_l50_r1_txt_allmasked", "k72_top1_l7_r0_img", "d128_k16_top8_l7_r2_txt"])
def test_hashes_carry_the_bits_of_the_eval_path_and_no_grad_keeps_no_record(case, monkeypatch):
    from xmh import ops
    from xmh._lib import lib
    from xmh.models import clip as C
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    h = _head(sd, D, layers, R, K, top_k)
    ct, tt = torch.tensor(cls).cuda(), torch.tensor(tok).cuda()
    outs = _encode(h, mod, ct.clone().requires_grad_(True), tt, mask)
    m = None if mask is None else torch.tensor(mask).cuda()
    before = ops.get_precision()
    ops.set_precision("f32x")
    try:
        monkeypatch.setattr(C, "NATIVE_FORWARD", False)                              # the per-primitive chain: gcl.run / lct.run
        _, ch, th, _ = h.encode_img(ct, tt) if mod == "img" else h.encode_txt(ct, tt, m)
        monkeypatch.setattr(C, "NATIVE_FORWARD", True)                               # and xmh_head_mith in exact mode
        _, ch2, th2, _ = h.encode_img(ct, tt) if mod == "img" else h.encode_txt(ct, tt, m)
    finally:
        ops.set_precision(before)
    assert torch.equal(outs[1].detach(), ch) and torch.equal(outs[2].detach(), th)
    assert torch.equal(ch, ch2) and torch.equal(th, th2)

    def boom(*a, **k):
        raise AssertionError("not under no_grad")
    real = lib.xmh_mith_train_forward
    seen = []

    def spy(*a):
        seen.append(a[10])                                                           # the saved pointer
        return real(*a)
    monkeypatch.setattr(lib, "xmh_mith_train_backward", boom)
    monkeypatch.setattr(lib, "xmh_mith_train_forward", spy)
    with torch.no_grad():
        z = _encode(h, mod, ct, tt, mask)
    assert seen and seen[-1] is None
    assert all(not o.requires_grad and o.grad_fn is None and torch.equal(o, w.detach()) for o, w in zip(z, outs))
    for p in h.parameters():
        p.requires_grad_(False)
    z = _encode(h, mod, ct, tt, mask)                                                # nothing to differentiate: the same plain forward
    assert seen[-1] is None and all(not o.requires_grad and torch.equal(o, w.detach()) for o, w in zip(z, outs))


def test_batch_of_one_keeps_its_row():
    case = "k8_top8_l7_r2_img"
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    h = _head(sd, D, layers, R, K, top_k)
    two = _encode(h, mod, torch.tensor(cls).cuda(), torch.tensor(tok).cuda(), None)
    one = _encode(h, mod, torch.tensor(cls[:1]).cuda(), torch.tensor(tok[:, :1]).cuda(), None)
    assert [tuple(o.shape) for o in one] == [(1, D), (1, K), (1, K), (K, 1, D)]     # the reference's torch.squeeze would return [K]
    assert torch.equal(one[1], two[1][:1]) and torch.equal(one[2], two[2][:1]) and torch.equal(one[3], two[3][:, :1])


def test_lta_aggregate_keeps_the_bits_of_its_earlier_kernel():
    """xmh_lta_aggregate's kernel body moved into csrc/xmh_lta.h: on the text tokens and mask of the MITH encode golden its output is
    the one the library gave before, stored in the golden file at generation time"""
    from xmh import ops
    G = MC.golden()
    scores, tok, mask, pe, top_k = MC.lta_inputs()
    out = ops.lta_aggregate(scores.cuda(), tok.cuda(), mask.cuda(), pe.cuda(), top_k).cpu().numpy()
    assert np.array_equal(MC.thin(out), G["lta_parent__thin"])
    assert float(zlib.crc32(np.ascontiguousarray(out).tobytes())) == float(G["lta_parent__crc"])


# 6 no host synchronisation, autograd's guards --------------------------------------------------------------------------------------
def test_forward_and_backward_do_not_synchronise():
    case = "d128_k16_top8_l7_r2_txt"
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    h = _head(sd, D, layers, R, K, top_k)
    ct, tt, m = torch.tensor(cls).cuda().requires_grad_(True), torch.tensor(tok).cuda().requires_grad_(True), torch.tensor(mask).cuda()
    u = [torch.tensor(x).cuda() for x in ups]
    run = lambda: sum((o * v).sum() for o, v in zip(h.encode_txt_train(ct, tt, m), u)).backward()      # noqa: E731
    run()                                                                            # warm the allocator's pools
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        run()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert ct.grad is not None and tt.grad is not None
    assert all(p.grad is not None for n, p in h.named_parameters() if not n.startswith("lct_i.") and not n.startswith("img_concept_proj"))


def test_in_place_parameter_write_and_double_backward_raise():
    case = "k8_top8_l7_r2_img"
    D, heads, layers, R, K, top_k, L, B, mod, mk = MC.CASES[case]
    sd, cls, tok, mask, ups = MC.case_inputs(case)
    h = _head(sd, D, layers, R, K, top_k)
    ct, tt = torch.tensor(cls).cuda().requires_grad_(True), torch.tensor(tok).cuda()
    outs = h.encode_img_train(ct, tt)
    with torch.no_grad():
        h.lct_i.hashing.fc_list[3].weight.mul_(2.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        outs[2].sum().backward()
    outs = h.encode_img_train(ct, tt)
    w = torch.ones_like(outs[1]).requires_grad_(True)                                # an upstream gradient with a graph of its own
    (g,) = torch.autograd.grad((outs[1] * w).sum() + outs[0].sum(), ct, create_graph=True)
    with pytest.raises(RuntimeError):                                                # the Function is once_differentiable
        g.sum().backward()


# 7 three BertAdam steps of the heads over a frozen backbone ------------------------------------------------------------------------
E2E = dict(steps=3, B=4, K=16, C=6, train_num=12, opt={"lr": 0.002, "backbone_lr": 0.0005, "e": 1e-3})
E2E_QUANTITIES = ("grad", "delta", "m", "v")


def _e2e_trainer(out_dir):
    import types
    import xmh.models  # noqa: F401
    import xmh.runners  # noqa: F401
    from xmh.common.register import registry
    from xmh.utils.config import Config
    small = "vision_layers=1,transformer_layers=1,vision_width=64,transformer_width=64,embed_dim=64,image_resolution=64"
    cfg = {"model": {"arch": "MITH", "clip_path": "synthetic:1814:" + small},
           "dataset": {"arch": "synthetic", "name": "synth", "num_classes": E2E["C"], "retrieval_num": 16, "max_word": 32, "image_resolution": 64,
                       "seed": 1814},
           "optimizer": dict(E2E["opt"]),
           "run": {"arch": "MITHTrainer", "output_dim": E2E["K"], "device": 0, "batch_size": E2E["B"], "num_workers": 0, "is_train": True,
                   "query_num": 8, "train_num": E2E["train_num"], "epochs": 1, "shuffle": False, "save_dir": str(out_dir), "log_dir": str(out_dir),
                   "seed": 1814}}
    t = registry.get_runner_class("MITHTrainer").from_config(cfg=Config(cfg), autorun=False)
    t.lines = []
    t.logger = types.SimpleNamespace(info=t.lines.append)
    return t


def _e2e_trajectory(init, feats, keeps, Y0, sims, rows, weights, hyper, heads, top_k, dtype):
    """the heads' training steps restated in `dtype`: init {(group, key): array}, feats / keeps / sims / rows per step -> per step
    dict(loss, grad, p, m, v) of numpy arrays keyed like init"""
    import bertadam_cases as AC
    import mith_loss_cases as ML
    from oracle import losses as OL
    npd = np.float64 if dtype == torch.float64 else np.float32
    out = []
    with ML.one_thread():
        Lf = {k: torch.tensor(v).to(dtype).requires_grad_(True) for k, v in init.items()}
        m = {k: np.zeros(v.shape, npd) for k, v in init.items()}
        v = {k: np.zeros(v_.shape, npd) for k, v_ in init.items()}
        Y = torch.as_tensor(Y0).to(dtype).clone()
        for s in range(len(feats)):
            for x in Lf.values():
                x.grad = None
            cls_i, tok_i, cls_t, tok_t, mask_t = feats[s]
            ti = {key: x for (g, key), x in Lf.items() if g in ("gcl", "i")}
            tt = {key: x for (g, key), x in Lf.items() if g in ("gcl", "t")}
            oi = MC.head_outputs(ti, torch.tensor(cls_i).to(dtype), torch.tensor(tok_i).to(dtype), None, heads, top_k, keeps[s][0])[0]
            ot = MC.head_outputs(tt, torch.tensor(cls_t).to(dtype), torch.tensor(tok_t).to(dtype), mask_t, heads, top_k, keeps[s][1])[0]
            Y[torch.as_tensor(rows[s])] = ot[2].detach()
            loss = OL.mith_terms((oi[0], ot[0], oi[1], ot[1], oi[2], ot[2], oi[3], ot[3]), Y, torch.as_tensor(sims[s]).to(dtype), weights)[0]
            loss.backward()
            rec = {"loss": float(loss.detach()), "grad": {}, "p": {}, "m": {}, "v": {}}
            lr = AC.lr_f64(hyper, s)
            for k, x in Lf.items():
                g, p = x.grad.numpy().copy(), x.detach().numpy().copy()
                if k[1] in ("hash_w", "hash_b"):                                     # K parameters of one row each: clipped one by one
                    for r in range(p.shape[0]):
                        p[r:r + 1], m[k][r:r + 1], v[k][r:r + 1], _ = AC.step_f64(p[r:r + 1], g[r:r + 1], m[k][r:r + 1], v[k][r:r + 1], lr, hyper)
                else:
                    p, m[k], v[k], _ = AC.step_f64(p, g, m[k], v[k], lr, hyper)
                assert p.dtype == npd
                with torch.no_grad():
                    x.copy_(torch.from_numpy(p))
                rec["grad"][k], rec["p"][k], rec["m"][k], rec["v"][k] = g, p, m[k].copy(), v[k].copy()
            out.append(rec)
    return out


def _e2e_errors(rec, ref, init):
    out = {}
    for q in E2E_QUANTITIES:
        for k in ref["p"]:
            a, b = (rec["p"][k] - init[k].astype(rec["p"][k].dtype), ref["p"][k] - init[k]) if q == "delta" else (rec[q][k], ref[q][k])
            key = (q, k[0] + "." + MC.kind_of(MC.grad_name(k[1])))
            out[key] = max(out.get(key, 0.0), MC.rel_err(a, b))
    return out


def test_three_bertadam_steps_of_the_heads_follow_the_float64_trajectory(tmp_path, monkeypatch):
    """forward_train_heads -> MITHTrainer.compute_loss -> backward -> BertAdam.step, three steps on the loader's three batches, against
    the float64 trajectory of the restatement chained with oracle.losses.mith_terms and bertadam_cases.step_f64.  The rule and the
    margins of tests/test_gpu_train_step.py: per quantity (the gradient as the optimiser receives it, delta = p - p_initial, next_m,
    next_v) and tensor kind, e <= TOL_FACTOR * e_ref with e_ref the float32 restatement against the float64 one on these very inputs,
    pooled over the steps; the loss within rtol 5e-5, atol 1e-6.  Both restatements use the keep-sets the device stored."""
    import bertadam_cases as AC
    import mith_loss_cases as ML
    from xmh.models import mith as M
    t = _e2e_trainer(tmp_path)
    model = t.model
    steps, B, K = E2E["steps"], E2E["B"], E2E["K"]
    raw = list(t.train_loader)
    assert len(raw) == steps and model.img_buffer_cls.shape == (E2E["train_num"], K)
    model.train()
    sd0 = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    named = {n[len("hash."):]: p for n, p in model.named_parameters() if n.startswith("hash.")}
    init = {}
    for n, p in named.items():
        g, key, row = MC.e2e_key(n)
        if row is None:
            init[(g, key)] = p.detach().cpu().double().numpy()
        else:
            init.setdefault((g, key), np.zeros((K,) + tuple(p.shape[1:]), np.float64))[row] = p.detach().cpu().double().numpy()[0]
    Y0 = model.img_buffer_cls.detach().cpu().clone()
    t.optimizer = t.build_optimizer(t.cfg.get("optimizer"), parameters=[{"params": list(model.hash.parameters()), "lr": E2E["opt"]["lr"]}])[0]
    hyper = dict(lr=E2E["opt"]["lr"], warmup=0.1, t_total=steps, schedule="warmup_cosine", b1=0.9, b2=0.98, e=E2E["opt"]["e"], weight_decay=0.2,
                 max_grad_norm=1.0)
    weights = {n: getattr(model, n) for n in ML.WEIGHTS}
    stored, real = [], M._head_forward

    def recording(*a, **k):
        outs, kept = real(*a, **k)
        if kept is not None:
            stored.append((M.saved_attention(kept[3], kept[4]) != 0).permute(2, 0, 1).cpu().numpy())
        return outs, kept
    monkeypatch.setattr(M, "_head_forward", recording)

    feats, sims, rows, port = [], [], [], []
    tl = torch.as_tensor(t.train_labels).float()
    for s, (image, text, kpm, label, index) in enumerate(raw):
        image, text, kpm = image.cuda(), text.cuda(), kpm.cuda()
        with torch.no_grad():
            cls_i, tok_i, _ = model.backbone.encode_image(image)
            cls_t, tok_t, _, new_mask = model.backbone.encode_text(text, key_padding_mask=kpm, masked_rows="zero")
        feats.append((cls_i.cpu().numpy(), tok_i.cpu().numpy(), cls_t.cpu().numpy(), tok_t.cpu().numpy(), new_mask.cpu().numpy()))
        sims.append(((tl @ torch.as_tensor(label).float().T) > 0).float().numpy())
        rows.append(np.asarray(index))
        outs = model.forward_train_heads(image, text, key_padding_mask=kpm)
        loss = t.compute_loss(*outs, label=label, index=index.numpy(), epoch=0, times=s + 1, global_step=s + 1)
        t.optimizer.zero_grad()
        loss.backward()
        pre = {n: p.grad.detach().clone() for n, p in named.items()}
        assert len(pre) == len(named) and all(p.grad is None for p in model.backbone.parameters())
        t.optimizer.step()
        rec = {"loss": float(loss.detach()), "grad": {}, "p": {}, "m": {}, "v": {}}
        for n, p in named.items():
            g, key, row = MC.e2e_key(n)
            st = t.optimizer.state[p]
            for q, val in (("grad", pre[n]), ("p", p.detach()), ("m", st["next_m"]), ("v", st["next_v"])):
                a = val.cpu().double().numpy()
                if row is None:
                    rec[q][(g, key)] = a
                else:
                    rec[q].setdefault((g, key), np.zeros_like(init[(g, key)]))[row] = a[0]
        port.append(rec)
    assert len(stored) == 2 * steps
    keeps = [(stored[2 * s], stored[2 * s + 1]) for s in range(steps)]
    for k, v in model.state_dict().items():                                          # the backbone is unchanged to the bit
        if k.startswith("backbone."):
            assert torch.equal(v.cpu(), sd0[k]), k
    heads, top_k = model.hash.lct_i.transformer.heads, model.hash.lct_i.lta.top_k
    args = (init, feats, keeps, Y0.numpy(), sims, rows, weights, hyper, heads, top_k)
    r64 = _e2e_trajectory(*args, torch.float64)
    r32 = _e2e_trajectory(*args, torch.float32)
    e_ref, e_port, lines, problems = {}, {}, [], []
    for s in range(steps):
        for key, e in _e2e_errors(r32[s], r64[s], init).items():
            e_ref[key] = max(e_ref.get(key, 0.0), e)
        for key, e in _e2e_errors(port[s], r64[s], init).items():
            e_port[key] = max(e_port.get(key, 0.0), e)
        lines.append("step %d loss %.8f f64 %.8f f32 %.8f lr %.3g" % (s, port[s]["loss"], r64[s]["loss"], r32[s]["loss"], AC.lr_f64(hyper, s)))
        if not abs(port[s]["loss"] - r64[s]["loss"]) <= 5e-5 * abs(r64[s]["loss"]) + 1e-6:
            problems.append((s, "loss", port[s]["loss"], r64[s]["loss"]))
    for key in sorted(e_ref):
        ratio = e_port[key] / e_ref[key] if e_ref[key] > 0 else (0.0 if e_port[key] == 0 else float("inf"))
        lines.append("%-6s %-22s e_port %.2e  e_ref %.2e  ratio %.2f" % (key + (e_port[key], e_ref[key], ratio)))
        if not e_port[key] <= TOL_FACTOR * e_ref[key]:
            problems.append((key, e_port[key], e_ref[key]))
    print("\n".join(lines))                                                          # every figure before the first assertion
    losses = [r["loss"] for r in port]
    assert all(np.isfinite(losses)) and len(set(losses)) == steps
    assert set(e_port) == set(e_ref) and not problems, (len(problems), problems[:12])
    assert any(np.abs(port[-1]["p"][k] - init[k]).max() > 0 for k in init)           # the steps moved the heads
