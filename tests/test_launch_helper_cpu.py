"""_hip._launch, the one function every wrapper of the ctypes binding hands its C-ABI launch to, against a stub library that
records what it is called with: argument conversion, the scratch pair, the stream in last place, the profile key and the
error it raises.  No GPU needed: the helper itself does not call need_f32_cuda, so CPU tensors do."""
import ctypes as C

import pytest
import torch

from galerkin_transformer import _hip

STREAM = 0x5EED


class _StubLib:
    """Every attribute is an entry point that records its positional arguments and returns ``rc``."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.rc
        return entry


@pytest.fixture
def stub(monkeypatch):
    s = _StubLib()
    monkeypatch.setattr(_hip, "lib", lambda: s)
    monkeypatch.setattr(_hip, "stream_ptr", lambda: STREAM)
    monkeypatch.setattr(_hip, "_prof", None)
    monkeypatch.setattr(_hip, "_DEBUG_SYNC", False)
    return s


def _drop(p):
    d = _hip.GtDropout()
    d.p, d.salt = p, 7
    return d


def test_argument_conversion(stub):
    t = torch.zeros(4)
    on, off = _drop(0.5), _drop(0.0)
    aff = _hip.GtResizeAffine()
    ref = C.byref(aff)
    _hip._launch("gt_probe", t, None, 3, 0.25, True, on, off, ref, 0xBEEF)
    (name, args), = stub.calls
    assert name == "gt_probe"
    assert args[0] == t.data_ptr() and type(args[0]) is int
    assert args[1] is None
    assert args[2] == 3 and type(args[2]) is int
    assert args[3] == 0.25 and type(args[3]) is float
    assert args[4] is True
    assert args[5]._obj is on                    # by reference, the caller's own structure
    assert args[6] is None                       # p == 0: "no dropout" is a null pointer
    assert args[7] is ref and args[7]._obj is aff
    assert args[8] == 0xBEEF
    assert args[9] == STREAM and len(args) == 10


def test_parameter_is_a_tensor(stub):
    w = torch.nn.Parameter(torch.zeros(2))
    _hip._launch("gt_probe", w)
    assert stub.calls[0][1] == (w.data_ptr(), STREAM)


def test_scratch_pair_then_stream(stub):
    ws = torch.zeros(48, dtype=torch.uint8)
    _hip._launch("gt_probe", 1, ws=ws)
    assert stub.calls[0][1] == (1, ws.data_ptr(), 48, STREAM)
    _hip._launch("gt_probe", 1, None, 0)         # an entry with a scratch pair that needs none: the caller passes NULL, 0
    assert stub.calls[1][1] == (1, None, 0, STREAM)


def test_stream_is_read_at_call_time(stub, monkeypatch):
    _hip._launch("gt_probe")
    monkeypatch.setattr(_hip, "stream_ptr", lambda: 99)
    _hip._launch("gt_probe")
    assert [a for _, a in stub.calls] == [(STREAM,), (99,)]


@pytest.mark.parametrize("key", [None, "gt_other_key"])
def test_key_names_the_error(stub, key):
    kw = {} if key is None else {"key": key}
    label = key or "gt_probe"                    # the key defaults to the symbol
    stub.rc = -4
    with pytest.raises(_hip.GtNotSupported, match="^" + label + ":"):
        _hip._launch("gt_probe", 1, **kw)
    stub.rc = -1
    with pytest.raises(_hip.GtError, match="^" + label + " failed") as e:
        _hip._launch("gt_probe", 1, **kw)
    assert not isinstance(e.value, _hip.GtNotSupported)
    assert [n for n, _ in stub.calls] == ["gt_probe", "gt_probe"]      # the symbol launched is `sym` whatever the key


def test_key_and_figures_reach_the_profile(stub, monkeypatch):
    """Under a Profile the same arguments are launched and the record carries key, flops, nbytes and shape."""
    seen = []

    def timed(key, flops, nbytes, fn, replay=None, shape=None):
        seen.append((key, flops, nbytes, shape))
        return fn()
    monkeypatch.setattr(_hip, "_timed", timed)
    monkeypatch.setattr(_hip, "_prof", object())
    t = torch.zeros(2)
    _hip._launch("gt_probe", t, 5)
    _hip._launch("gt_probe_affine", t, 5, key="gt_probe", flops=2.0, nbytes=8.0, shape=(1, 2))
    assert stub.calls == [("gt_probe", (t.data_ptr(), 5, STREAM)), ("gt_probe_affine", (t.data_ptr(), 5, STREAM))]
    assert seen == [("gt_probe", 0.0, 0.0, None), ("gt_probe", 2.0, 8.0, (1, 2))]
