"""CPU-side checks of the device-append boundary (no GPU calls): the header,
the binding list and the built library agree on srd_batch_append_device, its
14 arguments and its flag; and the Python layer carries the documented names.
csrc/srd_append.h (the range rule, the layout by one exclusive sum and the
refusals that the kernels and the host glue run) is checked against
srd_batch_layout by a stand-alone host program under ASan + UBSan,
tests/sanitize/append_check.cpp, which tests/test_sanitized_rules.py runs."""
import inspect
import os
import re
import subprocess

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "srd_batch_append_device"


def _header():
    return open(os.path.join(ROOT, "include", "srd_amd.h")).read()


def test_header_binding_and_library_agree():
    src = _header()
    m = re.search(r"\bint %s\s*\(([^;]*)\);" % NAME, src)
    assert m, NAME
    params = [p.strip() for p in re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",") if p.strip()]
    assert len(params) == 14, params
    # the order the issue fixes: blob, ranges, hashes, n, flags, the store as the delete call has it, outputs, stream
    names = [re.search(r"(\w+)$", p).group(1) for p in params]
    assert names == ["ctx", "d_payloads", "payloads_len", "d_src_off", "d_len", "d_key_hashes", "n", "flags", "tail",
                     "d_file", "file_cap", "new_tail", "d_meta_off_out", "stream"]
    f = re.search(r"#define SRD_APPEND_STREAM_RULE\s+(\d+)u?\b", src)
    assert f and int(f.group(1)) == srd_amd.APPEND_STREAM_RULE == 1
    assert NAME in srd_amd.EXPORTS
    if not os.path.exists(srd_amd.LIB_PATH):
        srd_amd.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", srd_amd.LIB_PATH], text=True)
    assert NAME in {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    L = srd_amd.lib()
    assert len(L.srd_batch_append_device.argtypes) == 14
    assert L.srd_batch_append_device.restype is not None
    # the 64-bit values are declared as such (a default int would truncate a tail or a length)
    import ctypes as C
    at = L.srd_batch_append_device.argtypes
    assert [at[i] for i in (2, 6, 8, 10)] == [C.c_uint64] * 4 and at[7] == C.c_uint32
    assert "waits a second time" in src  # the header says what the stream rule costs


def test_python_interface_names():
    assert callable(srd_amd.batch_append_device)
    D = srd_amd.DeviceStore
    for name in ("batch_write_device_with_key_hashes", "batch_write_device", "batch_copy", "batch_transfer",
                 "batch_rename", "copy", "transfer", "rename"):
        assert callable(getattr(D, name, None)), name
    sig = inspect.signature(D.batch_write_device_with_key_hashes)
    assert list(sig.parameters) == ["self", "hashes", "blob", "offs", "lens", "stream_rule"]
    assert sig.parameters["stream_rule"].default is False
    assert list(inspect.signature(D.batch_write_device).parameters) == ["self", "keys", "blob", "offs", "lens"]
    assert list(inspect.signature(D.batch_copy).parameters) == ["self", "keys", "target"]
    assert list(inspect.signature(D.batch_transfer).parameters) == ["self", "keys", "target"]
    assert list(inspect.signature(D.batch_rename).parameters) == ["self", "old_keys", "new_keys"]
