"""CPU-side checks of the payload-gather boundary (no GPU calls): the header,
the binding list and the built library agree on srd_payload_gather_device, its
14 arguments and its constants; and the Python classes carry the documented
names.  csrc/srd_gather.h (the range rule, the unit / chunk arithmetic and the
CRC combine the kernels run) is checked by a stand-alone host program under
ASan + UBSan, tests/sanitize/gather_check.cpp, which
tests/test_sanitized_rules.py runs."""
import os
import re
import subprocess

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "srd_payload_gather_device"


def _header():
    return open(os.path.join(ROOT, "include", "srd_amd.h")).read()


def _define(src, name):
    m = re.search(r"#define %s\s+(\d+)u?\b" % name, src)
    assert m, name
    return int(m.group(1))


def test_header_binding_and_library_agree():
    src = _header()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, src)
    assert m, NAME
    params = [p for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    assert len(params) == 14, params
    assert NAME in srd_amd.EXPORTS
    assert _define(src, "SRD_GATHER_CHUNK") == srd_amd.GATHER_CHUNK
    assert srd_amd.GATHER_CHUNK % 4096 == 0 and srd_amd.GATHER_CHUNK > 0
    assert _define(src, "SRD_GATHER_VERIFY_ONLY") == srd_amd.GATHER_VERIFY_ONLY == 1
    assert [_define(src, "SRD_GATHER_" + s) for s in ("NONE", "OK", "BAD_CRC", "BAD_RANGE")] == \
        [srd_amd.GATHER_NONE, srd_amd.GATHER_OK, srd_amd.GATHER_BAD_CRC, srd_amd.GATHER_BAD_RANGE] == [0, 1, 2, 3]
    if not os.path.exists(srd_amd.LIB_PATH):
        srd_amd.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", srd_amd.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = srd_amd.lib()
    assert len(L.srd_payload_gather_device.argtypes) == 14
    assert L.srd_payload_gather_device.restype is not None


def test_python_interface_names():
    assert callable(srd_amd.payload_gather_device)
    for name in ("data", "offs", "lens", "status", "crc_computed"):
        assert name in srd_amd.GatherResult.__init__.__code__.co_varnames, name
    for name in ("payloads", "is_valid_checksum"):
        assert hasattr(srd_amd.GatherResult, name), name
    assert hasattr(srd_amd.DeviceIndex, "batch_gather")
    for name in ("batch_gather", "batch_gather_hashed_keys", "verify", "iter_gather",
                 "_payloads", "batch_read", "batch_read_hashed_keys"):
        assert hasattr(srd_amd.DeviceStore, name), name
    r = srd_amd.GatherResult(None, [0, 64, 64, 64], [3, 0, 0], [srd_amd.GATHER_BAD_CRC, srd_amd.GATHER_NONE,
                                                                srd_amd.GATHER_BAD_RANGE], [1, 0, 0])
    assert r.is_valid_checksum() == [False, None, None] and len(r) == 3
