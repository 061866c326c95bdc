"""The batched InfoNCE form (impl 0 up to 1 024 padded rows: every directed pair's logits formed once and kept, one launch per
stage over all modalities / pairs) against the launch-by-launch slab form it replaces there (``ops.infonce_set_impl(1)``).  Both
run the same device code per output element -- same K order, same reduction order, same association of the two partners' dz
products -- so the comparison is ``torch.equal``, not a tolerance.  ``test_infonce_vs_oracle`` (test_10) gates the values themselves
against the CPU oracle."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SCALE = 1 / 0.07


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from bioscanclip.hip import ops as o
    return o


_INPUTS = {}
_REF = {}


def inputs(N, nmod, dup):
    """Embeddings and labels of one shape, made once and never written again."""
    key = (N, nmod, dup)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(1000 + N)
        zs = [torch.randn(N, 768, generator=g).cuda() for _ in range(nmod)]
        label = torch.arange(N)
        if dup:
            label = label // 3 * 3 if N > 8 else torch.tensor([0, 0, 1, 2, 3, 3, 3, 4])
        _INPUTS[key] = (zs, label.cuda())
    return _INPUTS[key]


def run(ops, impl, N, nmod, dup, rows=None, grad=True, ws=None, poison=False):
    """One call under ``impl``; returns (loss, [dz]) as fresh tensors.  The outputs start as NaN: every element must be written."""
    zs, label = inputs(N, nmod, dup)
    row0, nl = rows if rows else (0, N)
    if ws is None:
        ws = torch.empty(ops.infonce_workspace_floats(N, nmod), device="cuda")
    if poison:
        ws.fill_(float("nan"))
    loss = torch.full((1,), float("nan"), device="cuda")
    dz = [torch.full((nl, 768), float("nan"), device="cuda") for _ in range(nmod)] if grad else None
    ops.infonce_set_impl(impl)
    try:
        ops.infonce_fwd_bwd(zs, label, SCALE, loss, dz, row0=row0, n_local=nl, workspace=ws)
    finally:
        ops.infonce_set_impl(0)
    torch.cuda.synchronize()
    return loss, dz


def reference(ops, N, nmod, dup, rows=None, grad=True):
    """The slab form's result for a case: computed once, shared by the tests that compare against it."""
    key = (N, nmod, dup, rows, grad)
    if key not in _REF:
        _REF[key] = run(ops, 1, N, nmod, dup, rows, grad)
    return _REF[key]


def assert_same(got, ref, what):
    loss, dz = got
    rloss, rdz = ref
    assert torch.isfinite(rloss).all() and torch.equal(loss, rloss), (what, loss.item(), rloss.item())
    assert (dz is None) == (rdz is None)
    for i in range(len(dz or [])):
        assert torch.isfinite(rdz[i]).all(), (what, i)
        assert torch.equal(dz[i], rdz[i]), (what, i, (dz[i] - rdz[i]).abs().max().item())


# a padded Np (8, 200, 300), every pair slot (nmod = 3), the second-partner accumulate (nmod = 3), a slice that does not start at a
# tile edge (row0 = 50 / 100), Np = 512 (300) and the selection boundary (1 024 is the last size that takes the batched form)
@pytest.mark.parametrize("N,nmod,dup,rows", [(8, 2, False, None), (8, 3, True, None), (200, 3, True, None), (200, 3, True, (50, 100)),
                                             (256, 3, False, None), (300, 2, True, None), (300, 2, True, (100, 77)),
                                             (1024, 3, True, None)])
def test_batched_is_bit_equal_to_the_slab_form(ops, N, nmod, dup, rows):
    assert_same(run(ops, 0, N, nmod, dup, rows), reference(ops, N, nmod, dup, rows), (N, nmod, rows))


@pytest.mark.parametrize("N,nmod,dup", [(8, 3, True), (256, 3, False), (300, 2, True)])
def test_loss_only(ops, N, nmod, dup):
    """dz = None: the call ends after the loss; nothing of pass 2 is needed for it."""
    got = run(ops, 0, N, nmod, dup, grad=False)
    assert_same(got, reference(ops, N, nmod, dup, grad=False), (N, nmod))
    assert torch.equal(got[0], reference(ops, N, nmod, dup)[0])   # and it is the loss of the full call


def test_no_stale_or_unwritten_workspace(ops):
    """The workspace is NaN before every call, three modalities and then two share one buffer, and every call runs twice: nothing is
    read that the same call did not write, and nothing is left over from the call before (a NaN anywhere spreads into the result)."""
    N = 256
    ws = torch.empty(ops.infonce_workspace_floats(N, 3), device="cuda")
    assert ops.infonce_workspace_floats(N, 2) <= ws.numel()
    try:
        for nmod in (3, 2, 3, 2):
            ref = reference(ops, N, nmod, False)
            first = run(ops, 0, N, nmod, False, ws=ws, poison=True)
            second = run(ops, 0, N, nmod, False, ws=ws, poison=True)
            assert_same(first, ref, (nmod, "first"))
            assert_same(second, first, (nmod, "second"))
        sliced = run(ops, 0, N, 3, False, rows=(64, 100), ws=ws, poison=True)   # fewer rows in pass 2 than the call before wrote
        assert_same(sliced, reference(ops, N, 3, False, rows=(64, 100)), "slice after full")
    finally:
        ws.zero_()   # the block goes back to torch's caching allocator: leave no NaN for whoever gets it next


def test_above_one_slab_nothing_changed(ops):
    """N = 1 300 (Np = 1 536 > 1 024): impl 0 and impl 1 both take the launch-by-launch slab path."""
    assert_same(run(ops, 0, 1300, 2, True), reference(ops, 1300, 2, True), 1300)


def test_capture_and_replay(ops):
    """One call captured on one stream: the table and pointer arguments are baked into the graph's kernel nodes, and a replay
    (after the outputs and the workspace were overwritten) gives the eager result bit for bit."""
    N, nmod = 256, 3
    zs, label = inputs(N, nmod, False)
    eager = run(ops, 0, N, nmod, False)
    ws = torch.empty(ops.infonce_workspace_floats(N, nmod), device="cuda")
    loss = torch.zeros(1, device="cuda")
    dz = [torch.empty(N, 768, device="cuda") for _ in range(nmod)]
    ops.infonce_fwd_bwd(zs, label, SCALE, loss, dz, workspace=ws)   # the same buffers once outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.infonce_fwd_bwd(zs, label, SCALE, loss, dz, workspace=ws)
    try:
        for _ in range(2):
            ws.fill_(float("nan"))
            loss.fill_(float("nan"))
            for d in dz:
                d.fill_(float("nan"))
            graph.replay()
            torch.cuda.synchronize()
            assert_same((loss, dz), eager, "replay")
    finally:
        for t in [ws, loss] + dz:   # as above: no NaN left behind in memory that returns to the allocator
            t.zero_()


@pytest.fixture(scope="module", autouse=True)
def _drop_shared_tensors():
    """The inputs and references shared by the tests above live for this module only, and the large workspaces (113 MB each at
    N = 1 024) go back to the driver instead of staying in torch's cache for the rest of the session."""
    yield
    _INPUTS.clear()
    _REF.clear()
    if torch.cuda.is_available():
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
