"""The cross-batch memory (``model_config.memory_bank_size``) without a GPU: the host validation of ``bsclip_xbm_enqueue`` and
``bsclip_infonce_xbm_fwd_bwd`` (every limit is refused with -1 before any launch and the message names the argument), the size
functions, what the header documents, and the refusals of the criterion and of ``train_cl.py``."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "bioscan-clip_amd")
CONFIG = "model_config=lora_vit_lora_barcode_bert_ssl"

ONE = ctypes.c_void_p(16)                      # non-null, 16-byte aligned: never dereferenced on the host


def _ptrs(n, v=16):
    return (ctypes.c_void_p * n)(*[v] * n)


def _enqueue(h, nmod=2, N=8, D=768, Q=256, z="ok", labels=ONE, bank="ok", bank_labels=ONE, state=ONE, workspace=ONE):
    z = _ptrs(max(nmod, 1)) if z == "ok" else z
    bank = _ptrs(max(nmod, 1)) if bank == "ok" else bank
    return h.bsclip_xbm_enqueue(z, nmod, labels, N, D, bank, bank_labels, Q, state, workspace, None)


def _loss(h, nmod=2, N=8, D=768, Q=256, z="ok", labels=ONE, log_scale=ONE, bank="ok", bank_labels=ONE, state=ONE, loss=ONE, dz="ok",
          scale_out=ONE, workspace=ONE):
    z = _ptrs(max(nmod, 1)) if z == "ok" else z
    bank = _ptrs(max(nmod, 1)) if bank == "ok" else bank
    dz = _ptrs(max(nmod, 1)) if dz == "ok" else dz
    return h.bsclip_infonce_xbm_fwd_bwd(z, nmod, labels, N, D, log_scale, bank, bank_labels, Q, state, loss, dz, scale_out, workspace, None)


# what both entry points refuse, and the words the message must hold
SHARED = [(dict(D=512), ["D=512"]),
          (dict(nmod=1), ["nmod=1", "Too less element"]),
          (dict(nmod=4), ["nmod=4"]),
          (dict(N=0), ["N=0"]),
          (dict(N=1025, Q=2048), ["N=1025"]),
          (dict(Q=300), ["Q=300"]),
          (dict(Q=128), ["Q=128"]),
          (dict(Q=0), ["Q=0"]),
          (dict(Q=16640), ["Q=16640"]),
          (dict(N=512, Q=256), ["N=512", "Q=256"]),
          (dict(z=None), ["z is null"]),
          (dict(labels=None), ["labels"]),
          (dict(bank=None), ["bank is null"]),
          (dict(bank_labels=None), ["bank_labels"]),
          (dict(state=None), ["state_dev"]),
          (dict(state=ctypes.c_void_p(18)), ["state_dev", "4-B"]),
          (dict(workspace=None), ["workspace"]),
          (dict(workspace=ctypes.c_void_p(24)), ["workspace", "16-B"]),
          (dict(z=(ctypes.c_void_p * 2)(16, None)), ["z[1]"]),
          (dict(z=(ctypes.c_void_p * 2)(16, 24)), ["z[1]", "16-B"]),
          (dict(bank=(ctypes.c_void_p * 2)(16, None)), ["bank[1]"]),
          (dict(bank=(ctypes.c_void_p * 2)(16, 24)), ["bank[1]", "16-B"])]
LOSS_ONLY = [(dict(log_scale=None), ["log_scale_dev"]),
             (dict(log_scale=ctypes.c_void_p(18)), ["log_scale_dev", "4-B"]),
             (dict(loss=None), ["loss_out"]),
             (dict(scale_out=None), ["scale_out"]),
             (dict(dz=(ctypes.c_void_p * 2)(16, None)), ["dz[1]"]),
             (dict(dz=(ctypes.c_void_p * 2)(16, 24)), ["dz[1]", "16-B"])]


def test_every_limit_is_refused_before_any_launch_and_names_the_argument():
    """There is no GPU here: a call that got as far as a launch would not return -1 with a message of its own."""
    from bioscanclip.hip import lib
    h = lib.load()
    for fn, call, cases in (("bsclip_xbm_enqueue", _enqueue, SHARED), ("bsclip_infonce_xbm_fwd_bwd", _loss, SHARED + LOSS_ONLY)):
        for kw, words in cases:
            assert call(h, **kw) == -1, (fn, kw)
            msg = lib.last_error()
            assert fn in msg, (fn, kw, msg)
            for w in words:
                assert w in msg, (fn, kw, msg)


def test_size_functions():
    from bioscanclip.hip import lib
    h = lib.load()
    qs = [256, 512, 1024, 4096, 16384]
    banks = [h.bsclip_xbm_bank_floats(q) for q in qs]
    assert all(b >= q * 768 for b, q in zip(banks, qs))
    assert banks == sorted(banks) and len(set(banks)) == len(banks)
    assert all(b % 4 == 0 for b in banks)                                   # whole 16-byte units: banks laid side by side stay aligned
    for bad in (0, 128, 300, 16640, -256):
        assert h.bsclip_xbm_bank_floats(bad) == -1
    for nmod in (2, 3):
        for N in (1, 200, 256, 257, 1024):
            sizes = [h.bsclip_xbm_workspace_floats(N, q, nmod) for q in qs if q >= N]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes) and len(set(sizes)) == len(sizes)     # monotone in Q
        for q in (1024, 16384):
            sizes = [h.bsclip_xbm_workspace_floats(N, q, nmod) for N in (1, 5, 256, 257, 512, 1024)]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes)                                       # monotone in N
        assert h.bsclip_xbm_workspace_floats(256, 4096, 3) > h.bsclip_xbm_workspace_floats(256, 4096, 2)
    for bad in ((0, 256, 2), (1025, 2048, 2), (512, 256, 2), (8, 300, 2), (8, 256, 1), (8, 256, 4)):
        assert h.bsclip_xbm_workspace_floats(*bad) == -1, bad


def test_header_documents_the_entry_points_and_the_state_layout():
    from bioscanclip.hip import lib
    text = open(os.path.join(ROOT, "include", "bsclip.h")).read()
    block = text[text.index("Cross-batch memory"):text.index("/* ---- retrieval")]
    for name in ("bsclip_xbm_enqueue", "bsclip_infonce_xbm_fwd_bwd", "bsclip_xbm_bank_floats", "bsclip_xbm_workspace_floats"):
        assert re.search(r"\b" + name + r"\s*\(", block), name
    for words in ("int32 [2]", "(head, filled)", "j < filled", "Q * 768", "(head + i) % Q", "min(filled + N, Q)", "non-finite",
                  "No atomics", "Launches"):
        assert words in block, words
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)

    def ctype(a):
        if "* const*" in a:
            return ctypes.POINTER(ctypes.c_void_p)
        return ctypes.c_void_p if "*" in a else ctypes.c_int

    for name, names in (("bsclip_xbm_enqueue", ["z", "nmod", "labels", "N", "D", "bank", "bank_labels", "Q", "state_dev", "workspace",
                                                "stream"]),
                        ("bsclip_infonce_xbm_fwd_bwd", ["z", "nmod", "labels", "N", "D", "log_scale_dev", "bank", "bank_labels", "Q",
                                                        "state_dev", "loss_out", "dz", "scale_out", "workspace", "stream"])):
        m = re.search(r"int\s+" + name + r"\s*\((.*?)\)\s*;", hdr, flags=re.S)
        args = [" ".join(a.split()) for a in m.group(1).split(",")]
        assert [a.split()[-1].lstrip("*") for a in args] == names
        restype, argtypes = lib.SIGNATURES[name]
        assert restype is ctypes.c_int and list(argtypes) == [ctype(a) for a in args]
    assert lib.load().bsclip_abi_version() == 10


def test_criterion_refuses_more_than_one_rank_and_bad_sizes():
    import torch
    from bioscanclip.model.loss_func import ContrastiveLoss, MemoryBankContrastiveLoss
    crit = MemoryBankContrastiveLoss(memory_bank_size=512)
    assert isinstance(crit, ContrastiveLoss) and crit.memory_bank_size == 512
    assert not crit.state_dict() and list(crit.parameters()) == []
    assert int(crit.filled()) == 0 and crit.bank() is None
    crit.reset()                                                             # nothing allocated yet: a no-op
    with pytest.raises(ValueError, match="not built for more than one rank"):
        MemoryBankContrastiveLoss(memory_bank_size=512, world_size=2)
    for bad in (300, 128, 16640, 0):
        with pytest.raises(ValueError, match="memory_bank_size"):
            MemoryBankContrastiveLoss(memory_bank_size=bad)
    with pytest.raises(ValueError, match="Too less element for calculating the contrastive loss."):
        crit(torch.zeros(4, 768), None, None, torch.arange(4))
    with pytest.raises(RuntimeError, match="GPU"):                           # no CPU compute path
        crit(torch.zeros(4, 768), torch.zeros(4, 768), None, torch.arange(4))
    t = torch.nn.Parameter(torch.tensor(2.5))
    learn = MemoryBankContrastiveLoss(logit_scale=t, memory_bank_size=256)
    assert learn.logit_scale is t and list(learn.parameters()) == [] and not learn.state_dict()    # the model owns it


def test_train_cl_refuses_bad_sizes_before_the_model_is_built(monkeypatch):
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train_cl
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")
    monkeypatch.setattr(train_cl, "load_clip_model", lambda *a, **k: pytest.fail("the model was built"))
    with pytest.raises(ValueError, match="memory_bank_size=300"):
        train_cl.main([CONFIG, "model_config.memory_bank_size=300"])
    with pytest.raises(ValueError, match="smaller than the batch size"):
        train_cl.main([CONFIG, "model_config.memory_bank_size=256", "model_config.batch_size=512"])
    with pytest.raises(ValueError, match="memory_bank_size"):
        train_cl.main([CONFIG, "model_config.memory_bank_size=32768"])
    with pytest.raises(ValueError, match="memory_bank_size.*sigmoid"):
        train_cl.main([CONFIG, "model_config.memory_bank_size=256", "model_config.batch_size=8", "model_config.contrastive_loss=sigmoid"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="memory_bank_size.*not built for more than one rank"):
        train_cl.main([CONFIG, "model_config.memory_bank_size=256", "model_config.batch_size=8"])


def test_option_absent_means_off():
    sys.path.insert(0, os.path.join(PKG, "scripts"))
    import train_cl
    from bioscanclip.util.config import load_config
    cfg = load_config(os.path.join(PKG, "bioscanclip", "config"), [CONFIG])
    assert train_cl.memory_bank_size(cfg) is None
    cfg = load_config(os.path.join(PKG, "bioscanclip", "config"), [CONFIG, "model_config.memory_bank_size=4096"])
    assert train_cl.memory_bank_size(cfg) == 4096
