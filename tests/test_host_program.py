"""tests/host_program.py itself, on the CPU: the cache, what a failed compile and a failed run raise, that the one spelling of the
sanitizer flags is armed for both sanitizers, the two exchanges and the ABI probe.  The programs are one-liners."""
import os

import numpy as np
import pytest

from tests import golden_util as gu
from tests import host_program as hp

COPY = '#include <stdio.h>\nint main(int, char** v) { FILE *i = fopen(v[1], "rb"), *o = fopen(v[2], "wb"); int c; ' \
       "while ((c = fgetc(i)) != EOF) fputc(c, o); %s fclose(i); fclose(o); return 0; }\n"
# one int behind a 4-element heap array; 1 added to INT_MAX that the compiler cannot see (argv[1])
PAST_THE_END = "#include <cstdio>\n#include <cstdlib>\nint main(int n, char**) { int* volatile a = (int*)calloc(4, sizeof(int)); " \
               'int v = a[3 + n]; free(a); printf("%d\\n", v); return 0; }\n'
OVERFLOW = '#include <cstdio>\n#include <cstdlib>\nint main(int, char** v) { int x = atoi(v[1]); x += 1; printf("%d\\n", x); return 0; }\n'


def source(tmp_path, name, text):
    (tmp_path / name).write_text(text)
    return [str(tmp_path / name)]


def test_same_arguments_compile_once_and_any_flag_gives_another_file(tmp_path, monkeypatch):
    calls = []
    process = hp._process
    monkeypatch.setattr(hp, "_process", lambda cmd, **kw: calls.append(cmd) or process(cmd, **kw))
    src = source(tmp_path, "ok.cpp", "int main() { return 0; }\n")
    first = hp.build("ok", src)
    stamp = os.stat(first).st_mtime_ns
    assert hp.build("ok", src) == first and len(calls) == 1 and os.stat(first).st_mtime_ns == stamp
    others = [hp.build("ok", src, sanitize=True), hp.build("ok", src, opt="-O1"), hp.build("ok", src, define=["X=1"])]
    assert len({first, *others}) == 4 and len(calls) == 4 and all(os.path.isfile(p) for p in others)
    assert os.path.dirname(first) == hp.workdir() and {os.path.dirname(p) for p in others} == {hp.workdir()}


def test_a_compile_error_raises_with_the_diagnostic(tmp_path):
    with pytest.raises(RuntimeError, match="building broken failed") as e:
        hp.build("broken", source(tmp_path, "broken.cpp", "int main() { return no_such_name; }\n"))
    assert "no_such_name" in str(e.value) and "broken.cpp" in str(e.value)


def test_strict_makes_a_warning_an_error(tmp_path):
    src = source(tmp_path, "unused.cpp", "int main() { int unused_thing = 3; return 0; }\n")
    with pytest.raises(RuntimeError, match="unused_thing"):
        hp.build("unused", src)
    assert os.path.isfile(hp.build("unused", src, strict=False))


def test_a_nonzero_exit_raises_with_status_and_stderr(tmp_path):
    exe = hp.build("three", source(tmp_path, "three.cpp", '#include <cstdio>\nint main() { fprintf(stderr, "it went wrong\\n"); return 3; }\n'))
    with pytest.raises(RuntimeError) as e:
        hp.run(exe)
    assert "(3)" in str(e.value) and "it went wrong" in str(e.value) and os.path.basename(exe) in str(e.value)


@pytest.mark.parametrize("name,text,args,report", [("past_the_end", PAST_THE_END, [], "heap-buffer-overflow"),
                                                   ("overflow", OVERFLOW, [str(2 ** 31 - 1)], "signed integer overflow")],
                         ids=["address", "undefined"])
def test_the_sanitizer_flags_are_armed_and_cannot_be_downgraded(tmp_path, name, text, args, report):
    """Stand-alone host programs on the CPU.  Plain, both run clean; with SANITIZE each report ends the program, whatever the
    environment asks for."""
    src = source(tmp_path, name + ".cpp", text)
    assert hp.run(hp.build(name, src), args).returncode == 0
    lenient = dict(os.environ, ASAN_OPTIONS="halt_on_error=0", UBSAN_OPTIONS="halt_on_error=0")
    for env in (None, lenient):
        with pytest.raises(RuntimeError, match=report):
            hp.run(hp.build(name, src, sanitize=True), args, env=env)


def test_no_library_is_built_with_a_sanitizer(tmp_path, monkeypatch):
    monkeypatch.setattr(hp, "_process", lambda *a, **kw: pytest.fail("nothing may be compiled"))
    before = set(os.listdir(hp.workdir()))
    with pytest.raises(ValueError):
        hp.build("lib", source(tmp_path, "lib.cpp", "int f() { return 1; }\n"), sanitize=True, shared=True)
    assert set(os.listdir(hp.workdir())) == before


def test_binary_round_trip_end_of_file_and_clean_up(tmp_path):
    data = np.arange(1000, dtype=np.uint32)
    seen = []

    def write(f):
        seen.append(os.path.dirname(f.name))
        data.tofile(f)
    copy = hp.build("copy", source(tmp_path, "copy.cpp", COPY % ""))
    assert np.array_equal(hp.run_files(copy, write, lambda f: np.fromfile(f, np.uint32, data.size)), data)
    assert not os.path.exists(seen[0])
    one_more = hp.build("one_more", source(tmp_path, "one_more.cpp", COPY % "fputc(7, o);"))
    with pytest.raises(AssertionError):
        hp.run_files(one_more, write, lambda f: np.fromfile(f, np.uint32, data.size))
    assert not os.path.exists(seen[1])


def test_hex_exchange_keeps_every_bit():
    a = np.array([0x80000000, 0x7FC12345, 0xFFA00001, 0x00000001, 0x807FFFFF, 0x3F800000], np.uint32).view(np.float32)   # -0.0, NaNs with
    assert np.signbit(a[0]) and np.isnan(a[1]) and np.isnan(a[2]) and 0 < a[3] < np.finfo(np.float32).tiny              # payloads, denormals
    for width in (1, 3, 6):
        text = "".join(hp.hex_words(row) + "\n" for row in a.reshape(-1, width))
        got = hp.parse_hex_rows(text, width)
        assert got.dtype == np.uint32 and got.shape == (6 // width, width) and np.array_equal(got.reshape(-1), gu.bits(a))
    assert hp.hex_words(gu.bits(a)) == hp.hex_words(a)                       # words that are bit patterns already go out as they are
    with pytest.raises(AssertionError):
        hp.parse_hex_rows("00000001 00000002\n00000003\n", 2)                # a ragged row is an error, whatever the total


def test_abi_probe(monkeypatch):
    assert hp.c_values(["sizeof(mmdx_place_args)", "MMDX_PLACE_ON_DEVICE"]) == [40, 256]
    process = hp._process
    monkeypatch.setattr(hp, "_process", lambda cmd, **kw: pytest.fail("asked before: compiled already") if "-o" in cmd else process(cmd, **kw))
    assert hp.c_values(["sizeof(mmdx_place_args)", "MMDX_PLACE_ON_DEVICE"]) == [40, 256]
