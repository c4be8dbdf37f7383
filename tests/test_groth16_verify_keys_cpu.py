"""zk_bn254_groth16_verify_batch_keys / _dev without a GPU: both symbols are declared, listed and exported; every argument, key and stride error arrives
before a device is looked for, with its code (a malformed key with the host verifier's message and the key's index, a key_of out of range with its row) and
with the output buffers untouched; n_proofs = 0 is an empty result; otherwise the call is ZK_ERR_NO_DEVICE.  And the premises of
tests/test_gpu_groth16_verify_keys.py's own material (tests/groth16_keys_cases.py) under the host verifier, an error counting as a reject: every accept is
accepted under its own key, every wrong-key row is rejected, every member of every cross-key cancelling group is rejected alone, every freshly made key's
accept is accepted."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from noir_backend_using_gnark_amd import _lib
from noir_backend_using_gnark_amd import verify as zv
from tests import groth16_forge as gf
from tests import groth16_keys_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("zk_bn254_groth16_verify_batch_keys", "zk_bn254_groth16_verify_batch_keys_dev")


def _err():
    return (_lib.lib().zk_last_error() or b"").decode()


@pytest.fixture(scope="module")
def two():
    """two rows under two keys of two public inputs each"""
    ks = kc.np2_keys()
    return kc.Batch(kc.tiled_accepts([ks[0], ks[3]], [0, 1]))


def _raw(b, form, *, proofs=True, vks=True, lens=True, n_keys=None, key_of=None, pubs=True, pub_stride=None, acc=True, n_acc=True, n=None, proof_stride=128,
         keys=None):
    """the C entry with one argument replaced (False: a null pointer) -> (rc, *n_accepted); the _dev form gets host addresses, which no check reads.  The
    verdict buffer must come back as it went in"""
    raw = [k.bytes for k in b.keys] if keys is None else list(keys)
    ptrs, ls = (C.c_char_p * max(len(raw), 1))(*raw), (C.c_size_t * max(len(raw), 1))(*[len(x) for x in raw])
    ko = np.ascontiguousarray(b.key_of if key_of is None else key_of, dtype=np.uint32)
    pu = b.pubs()
    out, cnt = np.full(max(b.n, 1), 0xEE, np.uint8), C.c_size_t(77)
    n = b.n if n is None else n
    tail = (ptrs if vks else None, ls if lens else None, len(raw) if n_keys is None else n_keys, 0, _lib.vp(ko) if key_of is not False else None,
            _lib.vp(pu) if pubs else None, pu.shape[1] if pub_stride is None else pub_stride, _lib.vp(out) if acc else None, C.addressof(cnt) if n_acc else None)
    if form == "host":
        rc = _lib.lib().zk_bn254_groth16_verify_batch_keys(b.blob if proofs else None, n, *tail)
    else:
        buf = np.frombuffer(b.blob, np.uint8)
        rc = _lib.lib().zk_bn254_groth16_verify_batch_keys_dev(_lib.vp(buf) if proofs else None, proof_stride, n, *tail)
    assert (out == 0xEE).all()
    return rc, cnt.value


def test_symbols_declared_listed_and_exported():
    with open(os.path.join(ROOT, "include", "zkmi.h")) as f:
        hdr = f.read()
    for name in NAMES:
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in _lib.SYMBOLS and name in _lib.ARGTYPES
        assert hasattr(_lib.lib(), name)
    assert callable(zv.groth16_verify_batch_keys) and callable(zv.groth16_verify_batch_keys_dev)
    assert '"zkmi-groth16-batch-keys"' in hdr and '"zkmi-groth16-batch-keys-rows"' in hdr          # both derivations are stated


@pytest.mark.parametrize("form", ["host", "dev"])
def test_errors_come_before_a_device_is_looked_for(form, two):
    A, L = _lib.ZK_ERR_ARG, _lib.ZK_ERR_LEN
    # a null pointer that is read
    for what in ("proofs", "vks", "lens", "key_of", "pubs", "acc"):
        assert _raw(two, form, **{what: False}) == (A, 0), what
    assert _raw(two, form, n_acc=False)[0] == A
    # no key at all
    assert _raw(two, form, n_keys=0) == (A, 0)
    # a key_of out of range names its row and its value
    assert _raw(two, form, key_of=[1, 2]) == (A, 0)
    assert "key_of[1] = 2" in _err()
    assert _raw(two, form, key_of=[0xFFFFFFFF, 0]) == (A, 0)
    assert "key_of[0] = 4294967295" in _err()
    # pub_stride below the widest key's n_public, with more than one row -- an unused key counts
    assert _raw(two, form, pub_stride=1) == (L, 0)
    assert "pub_stride" in _err()
    wide = kc.Batch(two.rows, extra=(kc.npub_keys()[3],))
    assert wide.stride == 33 and _raw(wide, form, pub_stride=32) == (L, 0)
    # a malformed key: the host verifier's code and message, and which key
    c = two.rows[0][0]
    good = [k.bytes for k in two.keys]
    codes = []
    for bad in (good[1][:-1], good[1][:-32], b"\xff" * 32 + good[1][32:], good[1][:288] + (7).to_bytes(4, "big") + good[1][292:]):
        with pytest.raises(ValueError) as host:
            zv.groth16_verify(c.proof, bad, c.pub)
        ok = C.c_int(5)
        code = _lib.lib().zk_bn254_groth16_verify(C.c_char_p(c.proof), C.c_char_p(bad), C.c_size_t(len(bad)), C.c_int(0), _lib.vp(c.pub), C.c_size_t(len(c.pub)),
                                                  C.byref(ok))
        assert code in (A, L) and str(host.value) == _err()
        codes.append(code)
        if "witness size" in str(host.value):       # the key itself is well formed (a shorter K table): not an error of the key
            continue
        for at in (0, 1):
            keys = list(good)
            keys[at] = bad
            rc, cnt = _raw(two, form, keys=keys)
            assert rc == code and cnt == 0                                   # the host verifier's code for that key
            assert str(host.value) in _err() and "key %d: " % at in _err(), _err()
        with pytest.raises(ValueError, match="key 1"):
            zv.groth16_verify_batch_keys([c.proof], [good[0], bad], [0], [c.pub])
    assert A in codes
    if form == "dev":                                # a stride below the row, with more than one row
        assert _raw(two, form, proof_stride=127) == (A, 0)
        assert "proof_stride" in _err()
    with pytest.raises(ValueError):
        zv.groth16_verify_batch_keys(two.blob[:-1], good, two.key_of, two.pubs())      # not a whole number of proofs
    with pytest.raises(ValueError):
        zv.groth16_verify_batch_keys(two.blob, good, [0], two.pubs())                   # not one key index per proof
    with pytest.raises(ValueError):
        zv.groth16_verify_batch_keys(two.blob, [good[0], good[1].hex()], two.key_of, two.pubs())
    with pytest.raises(ValueError):
        zv.groth16_verify_batch_keys(two.blob, good, two.key_of, [two.rows[0][0].pub])  # not one row of public inputs per proof


@pytest.mark.parametrize("form", ["host", "dev"])
def test_no_proofs_is_an_empty_result(form, two):
    """the keys are still parsed; nothing else is read"""
    assert _raw(two, form, n=0, proofs=False, key_of=False, pubs=False, acc=False) == (_lib.ZK_OK, 0)
    assert _raw(two, form, n=0, n_keys=0, vks=False, lens=False, proofs=False, key_of=False, pubs=False, acc=False) == (_lib.ZK_OK, 0)
    rc, cnt = _raw(two, form, n=0, keys=[two.keys[0].bytes, b"\0" * 100])
    assert rc != _lib.ZK_OK and cnt == 0 and "key 1: " in _err()
    keys = [k.bytes for k in two.keys]
    if form == "host":
        got = zv.groth16_verify_batch_keys([], keys, [], np.zeros((0, 2, 4), np.uint64))
    else:
        got = zv.groth16_verify_batch_keys_dev(0, 128, 0, [k.hex() for k in keys], [], None, 2)
    assert got.dtype == bool and len(got) == 0


@pytest.mark.parametrize("form", ["host", "dev"])
def test_without_a_gpu_there_is_no_fallback(form, two):
    if _lib.device_count() > 0:
        pytest.skip("a GPU is present")
    assert _raw(two, form) == (_lib.ZK_ERR_NO_DEVICE, 0)
    one = kc.Batch(two.rows[:1])
    assert _raw(one, form, pub_stride=0) == (_lib.ZK_ERR_NO_DEVICE, 0)     # one row: its stride is not looked at
    none = kc.Batch([(kc.accepts_of(kc.npub_keys()[0])[0], None)])
    assert none.keys[0].n_public == 0
    assert _raw(none, form, pubs=False) == (_lib.ZK_ERR_NO_DEVICE, 0)      # no key has public inputs: the pointer may be null
    with pytest.raises(_lib.ZkmiError) as ei:
        zv.groth16_verify_batch_keys(two.blob, [k.bytes for k in two.keys], two.key_of, [c.pub for c, _ in two.rows])
    assert ei.value.code == _lib.ZK_ERR_NO_DEVICE


# ---------------------------------------------------------------------------------------------------------------- the GPU file's premises
def _host(case, key):
    try:
        return int(zv.groth16_verify(case.proof, key.bytes, case.pub))
    except ValueError:
        return 0


def test_accepts_are_accepted_under_their_own_key():
    labels = set()
    for k in kc.np2_keys() + kc.npub_keys():
        cs = kc.accepts_of(k)
        assert len(cs) >= 5
        for c in cs:
            assert _host(c, k) == 1, c.label
            labels.add(c.label.split(": ")[-1])
        assert _host(gf.reject_case(k), k) == 0
    for want in ("Ar at infinity", "Bs at infinity", "Krs at infinity", "IC at infinity", "public inputs + r"):
        assert want in labels, want
    ks = kc.np2_keys()
    assert ks[0] is gf.KEY and ks[1].ks[0] == 0 and ks[2].ks[1] == 0
    for c in gf.flag_loss_representatives():
        assert c.key is gf.KEY and _host(c, c.key) == 0


def test_wrong_key_rows_are_rejected():
    rows = kc.wrong_key_rows()
    assert len(rows) == 32
    for c, k in rows:
        assert c.key is not k and c.key.n_public == k.n_public
        assert _host(c, c.key) == 1 and _host(c, k) == 0, c.label


def test_cross_key_group_members_are_rejected_alone():
    groups = kc.cross_key_groups()
    assert len(groups) == 3
    for g in groups:
        a, b = g.members
        assert a.key is not b.key and a.expect == 0 and b.expect == 0
        assert sum(g.errors) % kc.R == 0 and all(e % kc.R for e in g.errors)
        assert _host(a, a.key) == 0 and _host(b, b.key) == 0, g.label


def test_freshly_made_keys_accept_their_proofs():
    keys, rej = kc.many_keys()
    assert len(keys) == kc.MANY == 300
    for k, c in keys:
        assert k.n_public == 1 and _host(c, k) == 1, c.label
    assert _host(rej, rej.key) == 0 and rej.key is keys[-1][0]
