"""The one call path from Python into the C ABI (hcflow_amd._lib.launch / Engine.launch) against a stub library: what reaches
the native function, under which device guard, on which stream, and what a failure raises. No GPU, no shared library."""
import contextlib
import ctypes as C
import types

import pytest
import torch

from hcflow_amd import _lib

STREAM = 0x5EED0
HANDLE = C.c_void_p(0xE0)


@pytest.fixture
def native(monkeypatch):
    """A stub in place of the loaded library plus recorders in place of the device guard and the stream accessor.
    native.events: ("enter", device) / ("exit",) of the guard and (entry name, args) of every native call, in order."""
    ev = []
    status = {}

    def entry(name):
        def fn(*args):
            ev.append((name, args))
            return status.get(name, 0)
        return fn

    @contextlib.contextmanager
    def guard(device):
        ev.append(("enter", device))
        yield
        ev.append(("exit",))

    stub = types.SimpleNamespace(hcf_probe=entry("hcf_probe"), hcf_train_select_tape=entry("hcf_train_select_tape"),
                                 hcf_last_error=lambda h: b"tape slot is busy")
    monkeypatch.setattr(_lib, "_lib", stub)
    monkeypatch.setattr(torch.cuda, "device", guard)
    monkeypatch.setattr(_lib, "current_stream", lambda device: STREAM)
    return types.SimpleNamespace(events=ev, status=status)


def _engine():
    eng = object.__new__(_lib.Engine)                  # no hcf_create: only the handle matters to launch()
    eng._h = None                                      # (__del__ then has nothing to destroy)
    return eng


def test_arguments_guard_and_stream(native):
    dev = torch.device("cuda", 0)
    t = torch.arange(6, dtype=torch.float32).reshape(2, 3)
    arr = (C.c_int32 * 2)(4, 5)
    vp = C.c_void_p(64)
    assert _lib.launch("hcf_probe", dev, t, None, 7, 0.25, arr, vp) is None
    assert [e[0] for e in native.events] == ["enter", "hcf_probe", "exit"]          # one guard per call, around the call
    assert native.events[0] == ("enter", dev)
    args = native.events[1][1]
    assert args[0] == t.data_ptr() and args[1] is None
    assert args[2] == 7 and type(args[2]) is int and args[3] == 0.25 and type(args[3]) is float
    assert args[4] is arr and args[5] is vp
    assert len(args) == 7 and isinstance(args[6], C.c_void_p) and args[6].value == STREAM      # the stream is the last argument


def test_an_int_device_is_that_gpu(native):
    _lib.launch("hcf_probe", 3)
    assert native.events[0] == ("enter", torch.device("cuda", 3))
    assert len(native.events[1][1]) == 1 and native.events[1][1][0].value == STREAM


def test_a_failure_names_the_entry_and_the_status(native):
    native.status["hcf_probe"] = -5
    with pytest.raises(_lib.HcfError) as e:
        _lib.launch("hcf_probe", torch.device("cuda", 0), 1)
    assert "hcf_probe" in str(e.value) and _lib.ERR_NAMES[-5] in str(e.value) and "HCF_ERR_SHAPE" in str(e.value)
    assert [ev[0] for ev in native.events] == ["enter", "hcf_probe"]                 # (raised inside the guard, which unwinds)
    with pytest.raises(_lib.HcfError) as e:                                          # with an engine: its last error joins the text
        _lib.launch("hcf_probe", 0, HANDLE, 1, engine=HANDLE)
    assert "hcf_probe" in str(e.value) and "tape slot is busy" in str(e.value)


def test_a_strided_tensor_never_reaches_the_library(native):
    with pytest.raises(_lib.HcfError) as e:
        _lib.launch("hcf_probe", torch.device("cuda", 0), 1, torch.zeros(4, 4).t())
    assert "hcf_probe" in str(e.value) and "argument 1" in str(e.value) and "contiguous" in str(e.value)
    assert native.events == []


def test_engine_launch_leads_with_the_handle_and_selects_the_tape_first(native):
    eng = _engine()
    eng._h = HANDLE
    t = torch.zeros(3)
    try:
        eng.launch("hcf_probe", 1, t, None, 2, tape=1)
        eng.launch("hcf_probe", 1, t)
    finally:
        eng._h = None
    names = [e[0] for e in native.events]
    assert names == ["enter", "hcf_train_select_tape", "hcf_probe", "exit", "enter", "hcf_probe", "exit"]   # same guard, tape first
    assert native.events[0] == ("enter", torch.device("cuda", 1))
    assert native.events[1][1] == (HANDLE, 1)
    args = native.events[2][1]
    assert args[0] is HANDLE and args[1:4] == (t.data_ptr(), None, 2) and args[4].value == STREAM and len(args) == 5
    assert native.events[5][1][:2] == (HANDLE, t.data_ptr())


def test_a_refused_tape_stops_before_the_entry(native):
    native.status["hcf_train_select_tape"] = -3
    eng = _engine()
    eng._h = HANDLE
    try:
        with pytest.raises(_lib.HcfError) as e:
            eng.launch("hcf_probe", 0, tape=0)
    finally:
        eng._h = None
    assert "hcf_train_select_tape" in str(e.value) and "HCF_ERR_STATE" in str(e.value)
    assert [ev[0] for ev in native.events] == ["enter", "hcf_train_select_tape"]
