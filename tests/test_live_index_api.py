"""CPU-side checks of the live-index boundary (no GPU calls): the header, the
binding list and the built library agree on the three new entry points, the
error code and the stats struct, and the Python classes carry the reference
method names."""
import ctypes as C
import os
import re
import subprocess

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["srd_index_table_apply_device", "srd_index_table_export_device", "srd_batch_delete_hashed_device"]


def test_header_binding_and_library_agree():
    src = open(os.path.join(ROOT, "include", "srd_amd.h")).read()
    for name in NEW:
        assert re.search(r"\bint %s\s*\(" % name, src), name
        assert name in srd_amd.EXPORTS
    m = re.search(r"#define SRD_ERR_FULL \((-?\d+)\)", src)
    assert m and int(m.group(1)) == srd_amd.SRD_ERR_FULL == -5
    fields = re.search(r"typedef struct \{([^}]*)\} srd_index_apply_stats;", src).group(1)
    assert re.findall(r"uint64_t (\w+);", fields) == [f for f, _ in srd_amd.ApplyStats._fields_]
    assert C.sizeof(srd_amd.ApplyStats) == 24
    if not os.path.exists(srd_amd.LIB_PATH):
        srd_amd.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", srd_amd.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert not [s for s in NEW if s not in exported]
    L = srd_amd.lib()
    assert len(L.srd_index_table_apply_device.argtypes) == 10
    assert len(L.srd_index_table_export_device.argtypes) == 7
    assert len(L.srd_batch_delete_hashed_device.argtypes) == 11


def test_python_interface_names():
    for name in ("apply", "remove", "export", "used", "__len__", "get_packed", "batch_read"):
        assert hasattr(srd_amd.DeviceIndex, name), name
    for name in ("open", "create", "batch_write", "batch_write_with_key_hashes", "batch_delete",
                 "batch_delete_key_hashes", "batch_read", "batch_read_hashed_keys", "exists", "len", "tail", "bytes"):
        assert hasattr(srd_amd.DeviceStore, name), name
