"""The document layer and the device half agree: for one stream per family (tests/doc_layer.py), a context on the device
reports the family and the flags that the stand-alone document-layer program (tests/host/doc_check.cpp, built here with
g++) printed for the same fields; the PDF kinds take their owner names; chunk planning knows all thirteen names; and the
context verifies a three-candidate list holding its password.  Thirteen small launches: chunk planning and the long-list
path are covered per family by the rest of the suite."""
import pytest

import doc_layer as D

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dprf():
    from dprf_amd import _lib
    assert _lib.device_count() >= 1, "no gfx950 device: GPU tests need the MI355X box"
    return _lib


@pytest.fixture(scope="module")
def printed(tmp_path_factory):
    """label -> (family, flags) as doc_check printed them."""
    exe = D.build_doc_check(tmp_path_factory.mktemp("doc_check"))
    rows = D.run(exe, [D.ctx_line(D.case(label)[0]) for label in D.LABELS])
    assert all(r[0] == "0" for r in rows)
    return dict((label, (r[1], int(r[3]))) for label, r in zip(D.LABELS, rows))


@pytest.mark.parametrize("label", D.LABELS)
def test_context_agrees_with_the_document_layer(dprf, printed, label):
    fields, pw, family, fmt = D.case(label)
    assert printed[label][0] == family
    with dprf.Context(fields, device=0) as ctx:
        assert (ctx.kernel, ctx.flags) == printed[label] and ctx.format == fmt
        assert dprf.plan_chunk(ctx.kernel, 0, 2 ** 62, 2 ** 62, 1) > 0
        hits, n, st = ctx.verify_list([pw + "x", pw, "x" + pw])
        assert (hits, n) == ([1], 1) and st["candidates"] == 3
        if fmt == 3:
            ctx.set_pdf_password("owner")
            assert ctx.kernel == family + "_owner"
            assert dprf.plan_chunk(ctx.kernel, 0, 2 ** 62, 2 ** 62, 1) > 0
            ctx.set_pdf_password("user")
            assert ctx.kernel == family
        else:
            with pytest.raises(dprf.DprfError) as ei:
                ctx.set_pdf_password("owner")                              # not a PDF context
            assert ei.value.code == dprf.E_INVALID and ctx.kernel == family


def test_chunk_planning_knows_every_name(dprf):
    for name in D.ALL_NAMES:
        assert dprf.plan_chunk(name, 0, 2 ** 62, 2 ** 62, 1) > 0, name
    for name in ("none", "pdf_r7", "office_std_owner", ""):
        assert dprf.plan_chunk(name, 0, 2 ** 62, 2 ** 62, 1) == 0, name
