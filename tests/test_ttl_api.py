"""CPU-side checks of the TTL cache's boundary (no GPU calls): the header, the
binding list, the built library and the ctypes argument lists agree on every
new entry and its parameter count; the four statuses are 0..3 in the header and
the module; the header names the reference code it replaces and says what each
call reads, writes and waits for; and the Python layer carries the documented
names.  csrc/srd_ttl.h over csrc/srd_table.h (the range rule, ttl_judge, the
saturating expiry, eviction's choice -- the code the kernels and the host glue
run) is checked by a stand-alone host program under ASan + UBSan,
tests/sanitize/ttl_check.cpp, which tests/test_sanitized_rules.py runs."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the prototypes as the interface fixes them
PARAMS = {
    "srd_namespace_hash_batch_device": ["ctx", "prefix_hash", "d_keys", "d_offs", "d_lens", "n", "d_ns_out", "d_hash_out",
                                        "stream"],
    "srd_namespace_hash_batch": ["ctx", "prefix_hash", "keys", "klen", "offs", "lens", "n", "ns_out", "hash_out"],
    "srd_ttl_resolve_device": ["ctx", "d_table", "table_bytes", "d_file", "file_len", "d_hashes", "n", "now", "d_start",
                               "d_end", "d_expiry", "d_status", "d_counts", "stream"],
    "srd_ttl_resolve_keys_device": ["ctx", "d_table", "table_bytes", "d_file", "file_len", "prefix_hash", "d_keys",
                                    "d_offs", "d_lens", "n", "now", "d_hashes_out", "d_start", "d_end", "d_expiry",
                                    "d_status", "d_counts", "stream"],
    "srd_ttl_evict_device": ["ctx", "d_table", "table_bytes", "used", "d_hashes", "d_status", "n", "tail", "d_file",
                             "file_cap", "new_tail", "n_evicted"],
    "srd_ttl_sweep_device": ["ctx", "d_table", "table_bytes", "used", "d_file", "tail", "file_cap", "now", "flags",
                             "new_tail", "stats"],
}
# the parameters the header declares as 64-bit values (a default int would truncate a time, a length or a count)
U64 = {"prefix_hash", "klen", "n", "table_bytes", "file_len", "now", "tail", "file_cap"}
U64_OUT = {"used", "new_tail", "n_evicted"}


def _header():
    return open(os.path.join(ROOT, "include", "srd_amd.h")).read()


def _proto(src, name):
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, src)
    assert m, name
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    return [re.sub(r"\s+", " ", p) for p in params]


@pytest.mark.parametrize("name", sorted(PARAMS))
def test_header_binding_and_library_agree(name):
    params = _proto(_header(), name)
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == PARAMS[name]
    assert name in srd_amd.EXPORTS
    if not os.path.exists(srd_amd.LIB_PATH):
        srd_amd.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", srd_amd.LIB_PATH], text=True)
    assert name in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    fn = getattr(srd_amd.lib(), name)
    at = fn.argtypes
    assert len(at) == len(names)
    assert fn.restype is C.c_int
    for p, k, t in zip(params, names, at):
        if k in U64:
            assert p == "uint64_t " + k and t == C.c_uint64, (p, t)
        elif k in U64_OUT:
            assert p == "uint64_t *" + k and t == C.POINTER(C.c_uint64), (p, t)
        elif k == "flags":
            assert p == "uint32_t flags" and t == C.c_uint32
        elif k == "stats":
            assert p == "srd_ttl_sweep_stats *stats" and t == C.POINTER(srd_amd.TtlSweepStats)
        else:
            assert "*" in p and t == C.c_void_p, (p, t)
    width = dict(zip(names, params))
    if "d_status" in width:
        assert width["d_status"] in ("uint8_t *d_status", "const uint8_t *d_status")


def test_status_values():
    src = _header()
    for i, k in enumerate(("NOT_FOUND", "LIVE", "EXPIRED", "TOO_SHORT")):
        m = re.search(r"#define\s+SRD_TTL_%s\s+(\d+)u" % k, src)
        assert m and int(m.group(1)) == i, k
        assert getattr(srd_amd, "TTL_" + k) == i
    m = re.search(r"#define\s+SRD_TTL_SWEEP_PLAN\s+(\d+)u", src)
    assert m and int(m.group(1)) == srd_amd.TTL_SWEEP_PLAN == 1
    # the stats struct: four u64 in the header's order
    td = re.search(r"typedef struct \{([^}]*)\} srd_ttl_sweep_stats;", src).group(1)
    assert re.findall(r"uint64_t (\w+);", td) == [n for n, _ in srd_amd.TtlSweepStats._fields_] == [
        "n_judged", "n_expired", "n_short", "next_expiry"]
    assert C.sizeof(srd_amd.TtlSweepStats) == 32
    assert srd_amd.TTL_PREFIX == bytes([0xF7, 0x74, 0x74, 0x6C, 0xFD])


def test_header_says_what_the_calls_are():
    src = _header()
    doc = src[src.index("---- TTL entries"): src.index("int srd_ttl_sweep_device")]
    assert "storage_cache_ext.rs:72-107" in doc and "namespace_hasher.rs:33-65" in doc and "constants.rs" in doc
    assert "Data too short to contain TTL" in doc
    # what waits and what does not
    res = doc[doc.index("read_with_ttl's decision for n key hashes"): doc.index("int srd_ttl_resolve_device")]
    assert "Asynchronous" in res and "reads only" in res and "[0, file_len)" in res
    assert "EXPIRED twice" in res  # the one deliberate difference from n sequential reads
    ev = doc[doc.index("srd_batch_delete_hashed_device restricted"): doc.index("int srd_ttl_evict_device")]
    assert "synchronises" in ev and "srd_padded_size(new" in ev and "last" in ev
    sw = doc[doc.index("The sweep:"):]
    assert "KEYS ARE NOT STORED" in sw and "EVERY live entry is judged as a TTL entry" in sw
    assert "only through the TTL writes" in sw and "left alone and counted" in sw and "synchronises" in sw
    assert "srd_ctx_device_bytes" in sw


def test_python_interface_names():
    D = srd_amd.DeviceStore
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(D.batch_write_with_ttl) == ["self", "keys", "values", "ttl_secs", "now"]
    assert sig(D.write_with_ttl) == ["self", "key", "value", "ttl_secs", "now"]
    assert sig(D.batch_write_stream_with_ttl) == ["self", "keys", "entries", "ttl_secs", "now"]
    assert sig(D.batch_read_with_ttl) == ["self", "keys", "now", "evict"]
    assert inspect.signature(D.batch_read_with_ttl).parameters["evict"].default is True
    assert sig(D.read_with_ttl) == ["self", "key", "now"]
    assert sig(D.batch_read_with_ttl_into) == ["self", "keys", "entries", "now", "evict"]
    assert sig(D.sweep_expired) == ["self", "now", "plan"]
    for name in ("batch_write_with_ttl", "batch_read_with_ttl", "read_with_ttl"):
        assert "storage_cache_ext.rs" in getattr(D, name).__doc__, name
    assert sig(srd_amd.NamespaceHasher.__init__)[:2] == ["self", "prefix"]
    assert sig(srd_amd.NamespaceHasher.namespace) == ["self", "key"]
    assert sig(srd_amd.NamespaceHasher.hash_batch) == ["self", "keys"]


def test_expiry_saturates_and_result_rule():
    import numpy as np
    S = srd_amd
    M = (1 << 64) - 1
    f = S.DeviceStore._ttl_expiries
    assert f(3, 60, 1000) == [1060] * 3
    assert f(3, [0, 1, M], M - 1) == [M - 1, M, M]
    assert f(1, M, M) == [M]
    with pytest.raises(ValueError):
        f(2, [1], 0)
    with pytest.raises(ValueError):
        f(1, -1, 0)
    # values(): the payloads without their 8 expiry bytes, None unless LIVE
    pay = b"\x01" * 8 + b"abc"
    data = type("T", (), {"cpu": lambda s: s, "numpy": lambda s: np.frombuffer(pay, np.uint8), "numel": lambda s: len(pay)})()
    g = S.GatherResult(data, np.array([0, 0, 64], np.uint64), np.array([0, 11], np.uint64),
                       np.array([S.GATHER_NONE, S.GATHER_OK], np.uint8), np.zeros(2, np.uint32))
    r = S.TtlReadResult(np.array([S.TTL_EXPIRED, S.TTL_LIVE], np.uint8), np.array([5, 99], np.uint64), g)
    assert len(r) == 2 and r.values() == [None, b"abc"] and r.is_valid_checksum() == [None, True] and r.n_evicted == 0
