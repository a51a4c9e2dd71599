"""Small host programs at test time: compile one with g++ / gcc, feed it rows, read its answer back.  Every test and reference
module that needs such a program goes through here; nothing in this module needs a GPU or the reference tree.

  * build() compiles a stand-alone program (or, shared=True, a library for ctypes) into ONE directory per process, removed at
    interpreter exit, and caches the result on its arguments;
  * run() runs a program and raises with the tail of its output when it fails; run_files() is the binary exchange
    (exe in.bin out.bin), hex_words() / parse_hex_rows() the text exchange of float bit patterns;
  * c_values() asks a C compiler what include/mmdx.h says: sizes and flag values as integers.
Nothing compiled here is committed.
"""
import atexit
import os
import shutil
import subprocess
import tempfile
import zlib

import numpy as np

from tests import golden_util as gu

TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
CSRC = os.path.join(ROOT, "simple_mmd_renderer_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
REF_INC = os.environ.get("REF_INC", "/root/reference/3rd_party/libmmd/include")    # as oracle/Makefile
# the one spelling of the sanitizer flags: no report of either sanitizer can be downgraded to a warning, by flag or environment
SANITIZE = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g")
COMPILE_TIMEOUT = 300

_built = {}        # build()'s arguments -> path
_workdir = []      # the directory of this process, once made


def reference_available() -> bool:
    """Are the reference's libmmd headers present?  (They are not on the GPU machines.)"""
    return os.path.isdir(os.path.join(REF_INC, "mmd"))


def workdir() -> str:
    if not _workdir:
        _workdir.append(tempfile.mkdtemp(prefix="mmdx_host_program_"))
        atexit.register(lambda d=_workdir[0], pid=os.getpid(): os.getpid() == pid and shutil.rmtree(d, ignore_errors=True))
    return _workdir[0]


def _process(cmd, **kw):
    return subprocess.run(cmd, capture_output=True, **kw)


def build(name, sources, *, cxx=True, c_std="c11", opt="-O2", strict=True, sanitize=False, shared=False, include=(), isystem=(),
          define=(), link=()) -> str:
    """Compile `sources` into the program `name` (shared=True: a library for ctypes) and return its path.  The same arguments give
    the same path without compiling again; any other flag gives another file.

    $CXX or g++ with -std=c++17, or (cxx=False) $CC or gcc with -std=<c_std>; -ffp-contract=off always.  strict=True is -Wall
    -Wextra -Werror, for the project's own code (the reference's headers may come in under `isystem`); strict=False is -w, for
    programs that are the reference's headers.  sanitize=True adds SANITIZE.  Sanitizers are for stand-alone programs with their
    own main: a library that will be loaded into python is never built with one here, so sanitize and shared together raise
    ValueError before anything is compiled."""
    if sanitize and shared:
        raise ValueError("%s: a library loaded into python is not built with a sanitizer; give the code a main of its own" % name)
    compiler = [os.environ.get("CXX", "g++"), "-std=c++17"] if cxx else [os.environ.get("CC", "gcc"), "-std=" + c_std]
    flags = [opt, "-ffp-contract=off"] + (["-Wall", "-Wextra", "-Werror"] if strict else ["-w"])
    flags += (list(SANITIZE) if sanitize else []) + (["-fPIC", "-shared"] if shared else [])
    flags += ["-I" + d for d in include] + [f for d in isystem for f in ("-isystem", d)] + ["-D" + d for d in define]
    key = (name, *compiler, *flags, *(str(s) for s in sources), *link)
    if key not in _built:
        out = os.path.join(workdir(), "%s_%d%s" % (name, len(_built), ".so" if shared else ""))
        r = _process(compiler + flags + [str(s) for s in sources] + ["-o", out] + list(link), text=True, timeout=COMPILE_TIMEOUT)
        if r.returncode != 0:
            raise RuntimeError("building %s failed:\n%s%s" % (name, r.stdout, r.stderr))
        _built[key] = out
    return _built[key]


def run(exe, args=(), *, stdin=None, timeout=300, env=None, text=True):
    """Run `exe args...` (an argument may be bytes) -> the CompletedProcess.  A non-zero exit raises RuntimeError with the program's
    name, its status and the END of its output: a sanitizer's report is the last thing on stderr."""
    r = _process([exe, *args], input=stdin, text=text, timeout=timeout, env=env)
    if r.returncode != 0:
        tail = lambda s, n: (s if text else s.decode(errors="replace"))[-n:]          # noqa: E731
        raise RuntimeError("%s failed (%d):\n%s%s" % (os.path.basename(exe), r.returncode, tail(r.stdout, 2000), tail(r.stderr, 4000)))
    return r


def run_files(exe, write, read, args=()):
    """The binary exchange: write(f) fills in.bin, `exe in.bin out.bin args...` runs, read(f) takes out.bin apart and must leave
    nothing unread -> what read returned.  The files are gone afterwards."""
    with tempfile.TemporaryDirectory(prefix="io_", dir=workdir()) as d:
        fin, fout = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
        with open(fin, "wb") as f:
            write(f)
        run(exe, [fin, fout, *args], text=False)          # an argument may be Shift-JIS: what the program echoes need not be UTF-8
        with open(fout, "rb") as f:
            out = read(f)
            assert f.read() == b""
    return out


def hex_words(array) -> str:
    """`array` (float32 values, or their bit patterns as uint32) as hex words, blank-separated: what the text drivers read."""
    array = np.asarray(array)
    return " ".join("%08x" % v for v in (array if array.dtype == np.uint32 else gu.bits(array)).reshape(-1))


def parse_hex_rows(stdout, width):
    """What the text drivers print, one row of `width` hex words per line -> u32 [rows, width]."""
    rows = [[int(v, 16) for v in line.split()] for line in stdout.splitlines()]
    assert all(len(r) == width for r in rows), sorted({len(r) for r in rows})
    return np.array(rows, np.uint32).reshape(-1, width)


def c_values(expressions, headers=("mmdx.h",)):
    """Each C expression over the project's headers (a sizeof, a flag) as the integer a C11 compiler gives it."""
    text = ("#include <stdio.h>\n" + "".join('#include "%s"\n' % h for h in headers) + "int main(void) {\n" +
            "".join('  printf("%%lld\\n", (long long)(%s));\n' % e for e in expressions) + "  return 0;\n}\n")
    src = os.path.join(workdir(), "c_values_%08x.c" % zlib.crc32(text.encode()))          # the same question is compiled once
    with open(src, "w") as f:
        f.write(text)
    return [int(v) for v in run(build("c_values", [src], cxx=False, include=[INCLUDE])).stdout.split()]
