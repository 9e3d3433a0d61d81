"""CPU: DSPH's HyP loss -- a float64 restatement of the reference expression (models/DSPH/loss/HyP.py:18-70) against goldens written by
the reference itself (oracle/make_golden_hyp.py), the codetable reader, the threshold's resolution order, and the argument checks of
xmh_hyp_loss / xmh_hyp_loss_grad, which run before any HIP call."""
import ctypes
import zipfile

import numpy as np
import pytest
import torch

from oracle.fixtures import aligned_host as _host, grads_close_rows as grads_close
from oracle.losses import HYP_CASES as CASES, hyp_oracle, load_hyp as load

SYNTH_CLIP = "synthetic:1814:vision_layers=1,transformer_layers=1"


@pytest.mark.parametrize("name", CASES)
def test_restatement_matches_the_reference(name):
    x, y, P, labels, threshold, alpha, loss, grads = load(name)
    if labels is None:
        labels = np.eye(x.shape[0])                            # reference object_function :79-81
    terms, gx, gy, gP = hyp_oracle(x, y, P, labels, threshold, alpha)
    assert np.allclose(terms[0], loss, rtol=2e-5, atol=1e-6), (name, terms[0], loss)
    for got, ref in zip((gx, gy, gP), grads):
        assert grads_close(got, ref), (name, np.abs(got - ref).max(), np.abs(ref).max())


def test_goldens_cover_the_degenerate_branches():
    """alpha 0, M empty, Z == 0 with M non-empty, an all-zero code row: each golden case exercises what its name says"""
    x, y, P, labels, threshold, alpha, _, _ = load("b100_k16_c80")
    assert hyp_oracle(x, y, P, labels, threshold, alpha)[0][5] > 0             # the regulariser is live in the COCO case
    for name in ("b64_k16_c80_alpha0", "b48_k16_c80_single", "b48_k16_c80_shared"):
        x, y, P, labels, threshold, alpha, _, _ = load(name)
        assert np.all(hyp_oracle(x, y, P, labels, threshold, alpha)[0][5:] == 0), name
    assert (load("b48_k16_c80_shared")[3].sum(1) > 1).any()
    assert np.any(np.abs(load("b40_k16_c80_zero_row")[0]).sum(1) == 0)
    assert load("b64_k128_c80")[4] == 0.0 and load("b100_k16_c80")[4] == 0.25    # codetable cells of (128, 80) and (16, 80)


# ---- the codetable reader ----------------------------------------------------------------------------------------------------
def _workbook(path, cells, shared=None, sheet_part="worksheets/data.xml"):
    """a minimal .xlsx: one sheet at xl/<sheet_part>, cells {"B2": 0.25, "C3": ("s", 0), ...}"""
    main = "http://schemas.openxmlformats.org/spreadsheetml/2006/main"
    rel = "http://schemas.openxmlformats.org/officeDocument/2006/relationships"
    rows = {}
    for ref, v in cells.items():
        rows.setdefault(int("".join(ch for ch in ref if ch.isdigit())), []).append((ref, v))
    xml_rows = []
    for r in sorted(rows):
        cs = []
        for ref, v in rows[r]:
            if isinstance(v, tuple):
                cs.append('<c r="%s" t="%s"><v>%s</v></c>' % (ref, v[0], v[1]))
            else:
                cs.append('<c r="%s"><v>%r</v></c>' % (ref, v))
        xml_rows.append('<row r="%d">%s</row>' % (r, "".join(cs)))
    with zipfile.ZipFile(path, "w") as z:
        z.writestr("xl/workbook.xml", '<workbook xmlns="%s" xmlns:r="%s"><sheets><sheet name="s" sheetId="1" r:id="rId7"/></sheets>'
                   '</workbook>' % (main, rel))
        z.writestr("xl/_rels/workbook.xml.rels", '<Relationships xmlns="http://schemas.openxmlformats.org/package/2006/relationships">'
                   '<Relationship Id="rId7" Type="%s/worksheet" Target="%s"/></Relationships>' % (rel, sheet_part))
        z.writestr("xl/" + sheet_part, '<worksheet xmlns="%s"><sheetData>%s</sheetData></worksheet>' % (main, "".join(xml_rows)))
        if shared is not None:
            z.writestr("xl/sharedStrings.xml", '<sst xmlns="%s">%s</sst>' % (main, "".join("<si><t>%s</t></si>" % s for s in shared)))


def test_codetable_reader_reads_the_cell_xlrd_would(tmp_path):
    from xmh.models import codetable
    p = str(tmp_path / "codetable.xlsx")
    # row 16 (0-based) is Excel row 17; ceil(log2(80)) = 7 is column H, ceil(log2(24)) = 5 is column F
    _workbook(p, {"B2": -1.0, "H17": 0.25, "F17": 0.0, "C17": -0.125, "H129": 0.0625, "D3": ("s", 1)}, shared=["a", "note"])
    assert codetable.read_cell(p, 1, 1) == -1.0                                  # B2 is (1, 1)
    assert codetable.read_cell(p, 2, 3) == "note"
    assert codetable.read_cell(p, 5, 5) is None
    assert codetable.hyp_threshold(p, 16, 80) == 0.25
    assert codetable.hyp_threshold(p, 16, 24) == 0.0
    assert codetable.hyp_threshold(p, 16, 4) == -0.125
    assert codetable.hyp_threshold(p, 128, 80) == 0.0625
    with pytest.raises(ValueError, match="holds no number"):
        codetable.hyp_threshold(p, 32, 80)


def test_threshold_resolution_order(tmp_path):
    from xmh.models.dsph import DSPH
    from xmh.utils.config import Config
    p = str(tmp_path / "codetable.xlsx")
    _workbook(p, {"H17": 0.25, "H33": 0.5})
    assert DSPH.resolve_threshold(Config({"threshold": 0.1, "codetable": p}), 16, 80) == 0.1
    assert DSPH.resolve_threshold(Config({"threshold": 0.1}), 16, 80, threshold=0.3) == 0.3
    assert DSPH.resolve_threshold(Config({"codetable": p}), 16, 80) == 0.25
    assert DSPH.resolve_threshold(Config({"codetable": p}), 32, 80) == 0.5
    assert DSPH.resolve_threshold(Config({}), 32, 80, codetable=p) == 0.5
    assert DSPH.resolve_threshold(Config({"threshold": 0.0, "codetable": p}), 16, 80) == 0.0    # an explicit 0 is a threshold
    assert DSPH.resolve_threshold(Config({}), 16, 80) is None and DSPH.resolve_threshold(None, 16, 80) is None
    m = DSPH.from_config(Config({"clip_path": SYNTH_CLIP, "codetable": p}), output_dim=16)
    assert m.hyp.threshold == 0.25 and m.hyp.alpha == 0.8


def test_dsph_without_a_threshold_constructs_and_the_loss_says_what_is_missing():
    from xmh.models.dsph import DSPH
    from xmh.utils.config import Config
    m = DSPH.from_config(Config({"clip_path": SYNTH_CLIP}), output_dim=16)
    assert m.hyp.threshold is None
    assert sorted(k for k in m.state_dict() if k.startswith("hyp")) == ["hyp.proxies"]        # no new parameter or buffer
    with pytest.raises(ValueError) as e:
        m.object_function(torch.rand(4, 16), torch.rand(4, 16), torch.ones(4, 80))
    assert "threshold" in str(e.value) and "codetable" in str(e.value)


def test_hyp_loss_rejects_cpu_tensors():
    from xmh.models.dsph import HyPProxies
    hyp = HyPProxies(numclass=5, output_dim=8, threshold=0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        hyp(torch.rand(3, 8), torch.rand(3, 8), torch.ones(3, 5))


# ---- C ABI argument checks (no GPU involved: each call returns before its first HIP call) ------------------------------------
def test_argument_errors_are_reported_without_a_gpu():
    from xmh._lib import lib
    assert lib.xmh_hyp_loss_ws_bytes(100, 16, 80) > 0 and lib.xmh_hyp_loss_ws_bytes(4096, 4096, 1024) > 0
    assert lib.xmh_hyp_loss_ws_bytes(0, 16, 80) == 0 and lib.xmh_hyp_loss_ws_bytes(4097, 16, 80) == 0
    need = lib.xmh_hyp_loss_ws_bytes(100, 16, 80)
    keep, p = _host(max(need, 1 << 16))
    _, out = _host(64)

    def loss(B=100, K=16, C=80, x=p, ws=p, ws_bytes=need, out8=out):
        return lib.xmh_hyp_loss(x, p, p, B, K, C, p, 0.25, 0.8, ws, ws_bytes, out8, None)

    def grad(B=100, K=16, C=80, x=p, ws=p, ws_bytes=need, gP=p):
        return lib.xmh_hyp_loss_grad(x, p, p, B, K, C, p, 0.25, 0.8, None, p, p, gP, 0, ws, ws_bytes, None)

    for call, name in ((loss, b"xmh_hyp_loss"), (grad, b"xmh_hyp_loss_grad")):
        assert call(B=0) == -22 and name + b": bad shape" in lib.xmh_last_error()
        assert call(K=-1) == -22 and call(C=0) == -22
        assert call(B=4097) == -95 and b"B <= 4096" in lib.xmh_last_error()
        assert call(K=4097) == -95 and call(C=1025) == -95
        assert call(x=None) == -22 and b"null pointer" in lib.xmh_last_error()
        assert call(ws=None) == -22
        assert call(ws_bytes=need - 1) == -22 and b"workspace" in lib.xmh_last_error()
        assert call(ws=ctypes.c_void_p(p.value + 8)) == -22 and b"aligned" in lib.xmh_last_error()
    assert loss(out8=None) == -22 and b"xmh_hyp_loss: null pointer" in lib.xmh_last_error()
    assert grad(gP=None) == -22 and b"xmh_hyp_loss_grad: null pointer" in lib.xmh_last_error()
    del keep
