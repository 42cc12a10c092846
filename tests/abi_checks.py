"""What the ABI tests of the libraries share (test_*_abi.py, test_ao_host.py, test_c_client.py, and the command-line refusals): a header as a strict C99 compiler
sees it against the ctypes mirror, a built library's exports and kernels, and a child process that has no device to touch."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def c99_probe(header, statements):
    """The words a C99 program prints that includes `header` and runs `statements` in main(): built with -std=c99 -pedantic -Wall -Werror, so the header is C99 too."""
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(src, "w") as f:
            f.write('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(void) {\n%s\nreturn 0; }\n' % (header, statements))
        r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INC, src, "-o", exe], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]   # (a field or constant the probe names and the header lacks fails here, by name)
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()


def struct_layout(header, structs, prelude=""):
    """{struct name: (sizeof, {field: offsetof})} of `structs` = {struct name: field names} as the C99 compiler lays them out. prelude: statements ahead of the probe's."""
    show = "".join('printf("%%d ", (int)sizeof(%s));' % s + "".join('printf("%%d ", (int)offsetof(%s, %s));' % (s, f) for f in fields) + "\n" for s, fields in structs.items())
    out = iter(int(v) for v in c99_probe(header, prelude + show))
    return {s: (next(out), {f: next(out) for f in fields}) for s, fields in structs.items()}


def assert_mirror(header, mirrors, prelude=""):
    """mirrors = {ctypes struct: field names}: the mirror has these fields in this order, and the header's struct of the same name their sizes and offsets.
    Returns [sizeof] in the order given."""
    layout = struct_layout(header, {t.__name__: fields for t, fields in mirrors.items()}, prelude)
    for t, fields in mirrors.items():
        assert [n for n, _ in t._fields_] == list(fields), t.__name__
        assert layout[t.__name__] == (C.sizeof(t), {f: getattr(t, f).offset for f in fields}), t.__name__
    return [C.sizeof(t) for t in mirrors]


def exported_names(path):
    """The dynamic symbols a built library defines."""
    if not os.path.exists(path):
        pytest.fail(f"{path} missing: __graft_entry__.build() builds it")
    r = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True)
    return {line.split()[-1] for line in r.stdout.splitlines() if line.strip()}


def assert_bound(lib, entry_points, names=None):
    """The loaded library's functions carry the table's result and argument types."""
    for name in entry_points if names is None else names:
        res, args = entry_points[name]
        assert getattr(lib, name).restype is res and getattr(lib, name).argtypes == args, name


def embedded_kernel_names(path):
    """{kernel symbol: .private_segment_fixed_size (scratch bytes)} of every kernel of the gfx950 code objects inside a built library."""
    readelf = next((p for p in ("/opt/rocm/lib/llvm/bin/llvm-readelf", "/opt/rocm/llvm/bin/llvm-readelf", shutil.which("llvm-readelf")) if p and os.path.exists(p)), None)
    if readelf is None:
        pytest.fail("llvm-readelf (ROCm's LLVM) not found: the kernels' metadata cannot be read")
    data = open(path, "rb").read()
    kernels, pos = {}, 0
    with tempfile.TemporaryDirectory() as tmp:
        while True:   # every embedded code object is an ELF for EM_AMDGPU (machine 0xE0); its size: section header offset + the section headers
            i = data.find(b"\x7fELF", pos)
            if i < 0:
                break
            pos = i + 4
            if data[i + 18:i + 20] != b"\xe0\x00":
                continue
            shoff = struct.unpack_from("<Q", data, i + 0x28)[0]; shentsize, shnum = struct.unpack_from("<HH", data, i + 0x3A)
            co = os.path.join(tmp, "co.elf")
            with open(co, "wb") as f:
                f.write(data[i:i + shoff + shentsize * shnum])
            notes = subprocess.run([readelf, "--notes", co], capture_output=True, text=True, check=True).stdout
            for block in notes.split("- .agpr_count:")[1:]:
                name = re.search(r"\.name:\s+(\S+)", block).group(1)
                kernels[name] = int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", block).group(1))
    return kernels


def no_device_env():
    """The environment of a child process that sees no GPU: whatever reaches for the device there fails (or does not return) instead of passing."""
    return dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")


PREAMBLE = r'''
import ctypes as C, sys
import numpy as np
sys.path.insert(0, %r)
from _pkg import import_pkg
pkg = import_pkg()
A = pkg._abi
lib = pkg.load_library()
REFUSALS = [0]
def refused(st, text=b""):
    REFUSALS[0] += 1
    assert st == A.PT_ERR_INVALID_ARG, (st, text, lib.lib.pt_last_error())
    assert text in lib.lib.pt_last_error(), (text, lib.lib.pt_last_error())
''' % ROOT


def run_without_device(body, timeout=300):
    """Runs `body` in a Python child that sees no GPU, behind a preamble that gives it pkg, A (the ctypes mirror), lib (the loaded libraries) and
    refused(status, text): one refusal -- PT_ERR_INVALID_ARG with `text` in pt_last_error(). The child must exit 0. Returns the number of refusals it checked."""
    r = subprocess.run([sys.executable, "-c", PREAMBLE + body + '\nprint("refused", REFUSALS[0])\n'], capture_output=True, text=True, env=no_device_env(), timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return int(re.search(r"^refused (\d+)$", r.stdout, re.M).group(1))
