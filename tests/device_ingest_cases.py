"""Shared by tests/test_gpu_device_ingest.py and the guard-mode script it starts: how a file is opened with the device
ingest switch off and on, what is compared (length, raw symbols, every level of the two chunks, what imc_last_ingest
says), the slab count the slab rule of csrc/ingest_tiles.hpp gives for a file, and the small cases that also run under
IMC_GUARD=1."""
import ctypes
import os

import numpy as np

from device_encode_cases import assert_same_chunk, compressible, tokens
from imcoalhmm_amd import Forwarder, _capi
from imcoalhmm_amd.hmm import set_device_encoding, set_device_ingest

WHITESPACE = b" \n\t\r\f\v"
MIN_SLAB = 4096
DEFAULT_SLAB = 4 << 20
SLAB_VARIABLE = "IMC_INGEST_SLAB_BYTES"


class slab_bytes(object):
    """``with slab_bytes(4096): ...`` - the slab size setting, which the library reads at every call (None: the default)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.before = os.environ.get(SLAB_VARIABLE)
        if self.value is None:
            os.environ.pop(SLAB_VARIABLE, None)
        else:
            os.environ[SLAB_VARIABLE] = str(self.value)

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop(SLAB_VARIABLE, None)
        else:
            os.environ[SLAB_VARIABLE] = self.before


def text_slabs(data, slab):
    """Slabs a text file of these bytes goes up in - every slab is cut after its last whitespace byte, the last one ends
    with the file - or None where a slab holds no whitespace (the device parser declines the file)."""
    slab = min(slab or DEFAULT_SLAB, max(len(data), MIN_SLAB))
    buf, pos, slabs = b"", 0, 0
    while True:
        take = min(slab - len(buf), len(data) - pos)
        buf += data[pos:pos + take]
        pos += take
        eof = pos == len(data)
        cut = len(buf) if eof else 1 + max(buf.rfind(bytes([c])) for c in WHITESPACE)
        if cut == 0:
            return slabs if eof else None
        slabs += 1
        buf = buf[cut:]
        if eof:
            return slabs


def pieces(total, slab):
    """Pieces a payload of `total` bytes goes up in (cache payloads; slab sizes are multiples of 16 there)."""
    slab = min((slab or DEFAULT_SLAB) & ~15, max((total + 15) & ~15, MIN_SLAB))
    return (total + slab - 1) // slab


def text_of(obs, sep=b" "):
    """The reference's file format: every symbol in decimal, each followed by `sep`."""
    return b"".join(b"%d" % int(v) + sep for v in obs)


def raw_symbols(f):
    return tokens(f, f.NSYM)[0]


def open_both(path, nsym, slab=None):
    """The same file as a chunk made with the switch off and one made with it on, and what imc_last_ingest says about the
    second."""
    with slab_bytes(slab):
        try:
            set_device_ingest(0)
            a = Forwarder(path, nsym)
            how_a = _capi.last_ingest()
            set_device_ingest(1)
            b = Forwarder(path, nsym)
            how_b = _capi.last_ingest()
        finally:
            set_device_ingest(0)
    assert how_a["path"] == "host" and how_a["columns"] == len(a), how_a
    return a, b, how_b


def assert_same_file(path, nsym, slab=None, path_name="text", want=None, what=None):
    """Switch 0 against switch 1 on one file: equal length, raw symbols and chunks at every level; the device path ran,
    with the slab count the slab rule gives.  `want`: the symbols the file was written from."""
    what = what or (os.path.basename(path), nsym, slab)
    data = open(path, "rb").read()
    a, b, how = open_both(path, nsym, slab)
    assert len(a) == len(b), (what, len(a), len(b))
    ra, rb = raw_symbols(a), raw_symbols(b)
    assert ra.size == rb.size == len(a) and (ra == rb).all(), (what, np.flatnonzero(ra != rb)[:8])
    if want is not None:
        assert rb.size == len(want) and (rb == np.asarray(want)).all(), what
    assert_same_chunk(a, b, what)
    assert how["path"] == path_name and how["columns"] == len(b), (what, how)
    if path_name == "text":
        assert how["slabs"] == text_slabs(data, slab) and how["bytes"] == len(data), (what, how, text_slabs(data, slab))
    elif path_name == "cache":
        assert how["slabs"] == pieces(len(data) - 24, slab) and how["bytes"] == len(data) - 24, (what, how)
    return a, b


def create_rc(path, nsym, mode, slab=None):
    """(return code, message, handle) of imc_obs_create_from_text with the switch at `mode`."""
    L = _capi.lib()
    h = ctypes.c_void_p()
    with slab_bytes(slab):
        try:
            set_device_ingest(mode)
            rc = L.imc_obs_create_from_text(os.fsencode(path), nsym, ctypes.byref(h))
            msg = L.imc_last_error() if rc else b""
        finally:
            set_device_ingest(0)
    if rc == 0:
        _capi.check(L.imc_obs_free(h))
    return rc, msg, h.value if rc else None


def assert_same_error(path, nsym, slab=None, code=None):
    host, device = create_rc(path, nsym, 0, slab), create_rc(path, nsym, 1, slab)
    assert host[0] != 0 and host[2] is None, host
    assert device == host, (os.path.basename(path), nsym, slab, host, device)
    if code is not None:
        assert host[0] == code, host
    return host


def small_cases(tmp, sizes=(4096, 4097, 8193), slab=4096):
    """Text, 2-bit cache and pairwise at sizes around a tile and a slab, with the smallest slab: the cases that run once
    more with every device buffer flush against an unmapped page."""
    from imcoalhmm_amd import prepare
    L = _capi.lib()
    set_device_encoding(0)
    for n in sizes:
        obs = compressible(n, seed=500 + n)
        t, c = os.path.join(tmp, "g%d.ziphmm" % n), os.path.join(tmp, "g%d.imc" % n)
        prepare.write_text(t, obs)
        prepare.write_cache(c, obs, 3)
        assert_same_file(t, 3, slab, "text", obs)
        assert_same_file(c, 3, slab, "cache", obs)
        rng = np.random.default_rng(n)
        s1, s2 = (bytes(rng.choice(np.frombuffer(b"ACGTacgtNn-", dtype=np.uint8), size=n)) for _ in range(2))
        want = np.empty(n, dtype=np.uint8)
        _capi.check(L.imc_encode_pairwise(s1, s2, n, want.ctypes.data_as(_capi._u8p)))
        with slab_bytes(2 * slab):
            f = Forwarder.from_sequences(s1, s2)
            how = _capi.last_ingest()
        assert how == {"path": "pairwise", "bytes": 2 * n, "slabs": (n + slab - 1) // slab, "columns": n}, how
        assert (raw_symbols(f) == want).all()
        assert_same_chunk(Forwarder.from_array(want, 3), f, ("pairwise", n))
