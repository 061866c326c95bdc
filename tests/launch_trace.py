"""The engines' launch sequences, recorded without a GPU and without the library.

``Recorder.install(setattr)`` replaces, through the caller's ``setattr(target, name, value)`` (a test passes ``monkeypatch.setattr``;
``recording()`` undoes its own), the few places where ``bioscanclip.hip.ops`` touches the device: ``lib.load`` returns an object whose
every attribute is a function that appends (entry point, arguments) to ``Recorder.calls`` and returns 0 (a small constant for the
``*_workspace_floats`` queries); ``ops._p`` turns a tensor into (buffer number in order of first appearance, byte offset into its
storage, dtype) instead of an address; the stream helpers hand out None / CPU scratch; ``torch.Tensor.is_cuda`` answers True.  Every
other host check of ``ops.py`` stays live: a trace is a list of calls that passed them.

``bsclip_epi_args`` / ``bsclip_fp8_args`` arrive by ``byref`` and are recorded field by field; their pointer fields hold plain
addresses, which are resolved against the storages seen so far (``ops.gemm`` / ``ops.gemm_fp8`` are wrapped to register their tensor
arguments first) -- an address inside no known storage raises.

``CASES`` names the engine configurations whose traces tests/golden/launch_trace.json pins (tools/gen_launch_trace_golden.py writes it,
tests/test_04_launch_trace_cpu.py compares); ``trace_case`` builds the engine of one case on CPU tensors and returns its forward
(+ backward) trace as one readable line per call.
"""
import contextlib
import ctypes

import torch

from helpers import skip_param_init

WORKSPACE_FLOATS = 64          # what every *_workspace_floats query answers
_POINTER_FIELDS = {"bias", "resid", "aux", "alpha", "a_aug", "b_aug"}


class _Buf:
    """A tensor argument: buffer number, byte offset into the buffer's storage, dtype."""

    def __init__(self, n, offset, dtype):
        self.n, self.offset, self.dtype = n, offset, dtype

    def __repr__(self):
        dt = "" if self.dtype is None else ":" + str(self.dtype).replace("torch.", "")
        return f"b{self.n}+{self.offset}{dt}"


class Recorder:
    def __init__(self):
        self.calls = []        # (entry point, [arguments])
        self._storages = []    # (base address, bytes, the storage itself: kept alive, so no address is ever reused)
        self._scratch = {}

    def reset(self):
        """Forget calls and buffer numbers (after an engine's constructor: a trace starts at the forward)."""
        self.calls, self._storages = [], []

    # ------------------------------------------------------------------------------------------------ buffers
    def _register(self, t):
        st = t.untyped_storage()
        base = st.data_ptr()
        for n, (b, _, _) in enumerate(self._storages):
            if b == base:
                return n
        self._storages.append((base, st.nbytes(), st))
        return len(self._storages) - 1

    def buf(self, t):
        if t is None:
            return None
        return _Buf(self._register(t), t.storage_offset() * t.element_size(), t.dtype)

    def _resolve(self, address, field):
        if not address:
            return None
        for n, (base, nbytes, _) in enumerate(self._storages):
            if base <= address < base + max(nbytes, 1):
                return _Buf(n, address - base, None)
        raise AssertionError(f"launch trace: struct field {field} = {address:#x} points into no tensor seen so far")

    def _struct(self, s):
        fields = []
        for name, _ in s._fields_:
            v = getattr(s, name)
            fields.append(f"{name}={self._resolve(v, name) if name in _POINTER_FIELDS else v!r}")
        return type(s).__name__ + "{" + ", ".join(fields) + "}"

    def _arg(self, a):
        if hasattr(a, "_obj") and isinstance(a._obj, ctypes.Structure):    # ctypes.byref(struct)
            return self._struct(a._obj)
        if a is None or isinstance(a, (_Buf, int, float)):
            return repr(a)
        raise AssertionError(f"launch trace: argument of unexpected type {type(a).__name__}")

    # ----------------------------------------------------------------------------------------------- the patches
    def install(self, setattr_):
        from bioscanclip.hip import lib, ops
        rec = self

        class _Lib:
            def __getattr__(self, name):
                def entry(*args):
                    rec.calls.append((name, [rec._arg(a) for a in args]))
                    return WORKSPACE_FLOATS if name.endswith("_workspace_floats") else 0
                return entry

        stand_in = _Lib()

        def _rowmajor(t, name):
            if t.dim() != 2 or t.stride(1) != 1:
                raise ValueError(f"{name}: expected a 2-D tensor with unit inner stride")
            return t.stride(0)

        def _stream_ws(tag, device, floats):
            ws = rec._scratch.get(tag)
            if ws is None or ws.numel() < floats:
                ws = rec._scratch[tag] = torch.empty(floats, dtype=torch.float32)
            return ws

        def registering(fn):
            def wrapped(*args, **kw):
                for t in list(args) + list(kw.values()):
                    if isinstance(t, torch.Tensor):
                        rec._register(t)
                return fn(*args, **kw)
            return wrapped

        setattr_(lib, "load", lambda: stand_in)
        setattr_(ops, "_p", rec.buf)
        setattr_(ops, "_stream", lambda: None)
        setattr_(ops, "_stream_ws", _stream_ws)
        setattr_(ops, "_rowmajor", _rowmajor)
        setattr_(ops, "_tables_ready", True)
        setattr_(ops, "gemm", registering(ops.gemm))
        setattr_(ops, "gemm_fp8", registering(ops.gemm_fp8))
        setattr_(torch.Tensor, "is_cuda", property(lambda self: True))

    def lines(self):
        return [f"{name}({', '.join(args)})" for name, args in self.calls]


@contextlib.contextmanager
def recording():
    """A Recorder installed for the duration of the block, with its own undo (tools; a test passes monkeypatch.setattr to install)."""
    missing, saved = object(), []

    def setattr_(target, name, value):
        saved.append((target, name, vars(target).get(name, missing)))
        setattr(target, name, value)

    rec = Recorder()
    try:
        rec.install(setattr_)
        yield rec
    finally:
        for target, name, old in reversed(saved):
            if old is missing:
                delattr(target, name)
            else:
                setattr(target, name, old)


# ------------------------------------------------------------------------------------------------------------ cases
def _mode(**kw):
    from bioscanclip.hip.engine import EngineMode
    base = dict(grad_stream_bf16=True, resid_stream_bf16=True, patch_split=True, exact=False, attn_keep_bits=True, attn_lora=True,
                fp8=False, fp16=False, full_ft=False)
    base.update(kw)
    return EngineMode(**base)


F32_STREAMS = dict(grad_stream_bf16=False, resid_stream_bf16=False)
MODES = {"default": {}, "f32_streams": F32_STREAMS, "exact": dict(F32_STREAMS, exact=True), "fp8": dict(fp8=True), "fp16": dict(fp16=True),
         "full_ft": dict(full_ft=True), "attn_lora_off": dict(attn_lora=False)}

# name -> (tower, mode name, B, train (dropout sites live; False = eval()), backward)
CASES = {f"vit_d3_B2_{m}": ("vit", m, 2, True, True) for m in MODES}
CASES["vit_d3_B3_default"] = ("vit", "default", 3, True, True)
CASES["vit_d3_B2_default_eval_forward"] = ("vit", "default", 2, False, False)
CASES.update({f"dna_L2_S133_B2_{m}": ("dna", m, 2, True, True) for m in ("default", "exact", "fp8", "full_ft")})
CASES["dna_L2_S133_B2_fp16_forward"] = ("dna", "fp16", 2, False, False)
CASES["txt_S20_B2_default_masked"] = ("txt", "default", 2, True, True)

VIT_DEPTH, DNA_LAYERS, DNA_S, TXT_S = 3, 2, 133, 20


def _engine(tower, mode):
    """(engine, forward arguments) of one tower on CPU tensors; the module's parameters are uninitialised memory (no kernel runs)."""
    from bioscanclip.hip import engine, engine_ft
    from bioscanclip.model import arch
    cpu = torch.device("cpu")
    if tower == "vit":
        from bioscanclip.model.image_encoder import LoRA_ViT_timm
        with skip_param_init():
            m = LoRA_ViT_timm(arch.VisionTransformerParams(depth=VIT_DEPTH), r=4, num_classes=768)
        return (engine_ft.ViTEngineFT if mode.full_ft else engine.ViTEngine)(m, cpu, mode), None
    lora_layer = [] if mode.full_ft else None     # full fine-tuning: the BERT towers carry no LoRA branch
    cls = engine_ft.BertEngineFT if mode.full_ft else engine.BertEngine
    if tower == "dna":
        from bioscanclip.model.dna_encoder import LoRA_barcode_bert
        with skip_param_init():
            m = LoRA_barcode_bert(arch.BertForMaskedLMParams(arch.barcode_bert_config(num_hidden_layers=DNA_LAYERS)), r=4,
                                  num_classes=768, lora_layer=lora_layer)
        bert = m.lora_barcode_bert
        return cls(bert.bert, "mlm_softmax_mean", (bert.cls.predictions.transform, bert.cls.predictions.decoder), cpu, mode), DNA_S
    from bioscanclip.model.language_encoder import LoRA_bert
    with skip_param_init():
        m = LoRA_bert(arch.BertModelParams(arch.bert_small_config()), r=4, num_classes=768, lora_layer=lora_layer)
    return cls(m.lora_bert, "mean_proj", (m.proj,), cpu, mode), TXT_S


def trace_case(name, setattr_=None):
    """The launch trace of case ``name``: one line per C-ABI call of one forward (and backward).  ``setattr_``: monkeypatch.setattr (a
    test), or None for patches that are undone on return."""
    tower, mode_name, B, train, backward = CASES[name]
    with contextlib.ExitStack() as stack:
        if setattr_ is None:
            rec = stack.enter_context(recording())
        else:
            rec = Recorder()
            rec.install(setattr_)
        torch.manual_seed(0)     # the BERT dropout seeds derive from torch.initial_seed()
        eng, S = _engine(tower, _mode(**MODES[mode_name]))
        eng.training = train
        rec.reset()
        if tower == "vit":
            args = (torch.zeros(B, 3, 224, 224),)
        else:
            mask = torch.ones(B, S, dtype=torch.int64) if tower == "txt" else None
            args = (torch.zeros(B, S, dtype=torch.int64), None, mask)
        out = eng.forward(*args)
        if backward:
            eng.backward(torch.zeros_like(out))
        return rec.lines()
