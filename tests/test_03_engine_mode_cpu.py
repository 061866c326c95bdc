"""CPU checks of the engines' mode snapshot (hip/engine.py EngineMode): the module globals and the ``hip_*`` module attributes are
the request, ``wanted_mode`` reads all of them, and each of the three setters drops a module's engine while parking it so that the
engine built next inherits its flat parameter / gradient buffer."""
import pytest
import torch

from bioscanclip.hip import engine

GLOBALS = {"GRAD_STREAM_BF16": "grad_stream_bf16", "RESID_STREAM_BF16": "resid_stream_bf16", "PATCH_SPLIT": "patch_split",
           "EXACT_FORWARD": "exact", "ATTN_KEEP_BITS": "attn_keep_bits", "ATTN_LORA": "attn_lora"}
ATTRS = {"fp8": ("hip_precision", "fp8"), "fp16": ("hip_operands", "fp16"), "full_ft": ("hip_full_ft", True)}


def _encoder():
    m = torch.nn.Module()
    m.lora_vit = torch.nn.Linear(2, 2)
    m._engine = None          # as the encoder modules' constructors leave it
    return m


def test_mode_fields_are_the_inputs_that_shape_an_engine():
    assert engine.EngineMode._fields == tuple(GLOBALS.values()) + tuple(ATTRS)


@pytest.mark.parametrize("name", list(GLOBALS))
def test_wanted_mode_reflects_each_global(name, monkeypatch):
    m = _encoder()
    base = engine.wanted_mode(m)
    assert base == engine.wanted_mode(m) and hash(base) == hash(engine.wanted_mode(m))     # two equal requests compare equal
    for value in (False, True):
        monkeypatch.setattr(engine, name, value)
        mode = engine.wanted_mode(m)
        assert getattr(mode, GLOBALS[name]) is value
        assert mode == base._replace(**{GLOBALS[name]: value})     # ... and nothing else moved
        assert (mode != base) == (value != getattr(base, GLOBALS[name]))


@pytest.mark.parametrize("field", list(ATTRS))
def test_wanted_mode_reflects_each_module_attribute(field):
    m, other = _encoder(), _encoder()
    base = engine.wanted_mode(m)
    assert not getattr(base, field)
    setattr(m, *ATTRS[field])
    assert engine.wanted_mode(m) == base._replace(**{field: True}) != base
    assert engine.wanted_mode(other) == base      # the request is per module


def test_every_single_switch_gives_a_different_mode():
    base = engine.wanted_mode(_encoder())
    seen = {base}
    for field in engine.EngineMode._fields:
        seen.add(base._replace(**{field: not getattr(base, field)}))
    assert len(seen) == 1 + len(engine.EngineMode._fields)
    with pytest.raises(AttributeError):
        base.exact = True       # a snapshot: immutable


def test_set_parity_mode_sets_the_request(monkeypatch):
    for name in ("GRAD_STREAM_BF16", "RESID_STREAM_BF16", "EXACT_FORWARD"):
        monkeypatch.setattr(engine, name, getattr(engine, name))     # restored at teardown
    engine.set_parity_mode(0)
    m = _encoder()
    for level, (streams16, exact) in {1: (False, False), 2: (False, True), 0: (True, False), True: (False, False)}.items():
        prev = (engine.GRAD_STREAM_BF16, engine.RESID_STREAM_BF16)
        assert engine.set_parity_mode(level) == prev
        mode = engine.wanted_mode(m)
        assert (mode.grad_stream_bf16, mode.resid_stream_bf16, mode.exact) == (streams16, streams16, exact)


class _Engine:     # stands in for the engine of a module that has run: the setters only move it
    pass


@pytest.mark.parametrize("setter", ["set_precision", "set_operand_format", "set_parity_mode"])
def test_each_setter_drops_the_engine_and_parks_it(setter, monkeypatch):
    for name in ("GRAD_STREAM_BF16", "RESID_STREAM_BF16", "EXACT_FORWARD"):
        monkeypatch.setattr(engine, name, getattr(engine, name))
    model = torch.nn.ModuleDict({"image_encoder": _encoder()})
    m = model["image_encoder"]
    calls = {"set_precision": lambda: engine.set_precision(model, "fp8"), "set_operand_format": lambda: engine.set_operand_format(model, "fp16"),
             "set_parity_mode": lambda: engine.set_parity_mode(1, model)}
    calls[setter]()          # a module that has not run yet: nothing to park
    assert m._engine is None and getattr(m, "_engine_prev", None) is None
    m._engine = first = _Engine()
    calls[setter]()
    assert m._engine is None and m._engine_prev is first
    calls[setter]()          # a second switch before any forward keeps the parked engine
    assert m._engine is None and m._engine_prev is first
