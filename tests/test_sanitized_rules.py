"""The stand-alone ASan + UBSan host programs of tests/sanitize (CPU only;
nothing is loaded into Python): one NAME_check per rule header of csrc -- the
arithmetic the kernels and the host glue run, compiled for the host.  What each
program covers stands in the first comment of its .cpp; this module builds
each, runs it and reads its verdict line "NAME ok: M checks[, detail]".
(host_fuzz, the program over the host parsers of untrusted store bytes, takes
the golden fixtures as arguments and runs through run_sanitized from
tests/test_host_tools.py.)"""
import os
import re
import subprocess

import pytest

import srd_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "sanitize")
CHUNK = "chunk %d," % srd_amd.GATHER_CHUNK

# program, what its output must hold besides the verdict
PROGRAMS = [
    ("part_check", []),
    ("fin_check", []),
    ("table_check", []),
    ("append_check", [CHUNK]),
    ("gather_check", [CHUNK]),
    ("segments_check", [CHUNK]),
    ("scatter_check", [CHUNK]),
    ("ttl_check", []),
    ("rows_check", []),
]


def run_sanitized(name, args=()):
    """Build tests/sanitize/build/NAME, run it under ASan + UBSan and return its stdout: the program exited 0,
    printed "NAME ok" and evaluated at least one check."""
    subprocess.check_call(["make", "-s", "-C", DIR, "build/" + name])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([os.path.join(DIR, "build", name), *args], capture_output=True, text=True, env=env, timeout=600)
    # a sanitizer report names the fault at its head and the program's own lines come last: show both ends
    err = p.stderr if len(p.stderr) <= 5000 else p.stderr[:2000] + "\n[...]\n" + p.stderr[-3000:]
    assert p.returncode == 0 and name + " ok" in p.stdout, "stdout: %s\nstderr: %s" % (p.stdout[-1000:], err)
    m = re.search(r"^%s ok: (\d+) checks" % name, p.stdout, re.M)
    assert m and int(m.group(1)) > 0, p.stdout[-1000:]  # a program whose loops run zero times has checked nothing
    return p.stdout


@pytest.mark.parametrize("name,wanted", PROGRAMS, ids=[p[0] for p in PROGRAMS])
def test_sanitized(name, wanted):
    out = run_sanitized(name)
    for w in wanted:
        assert w in out, (w, out[-1000:])
