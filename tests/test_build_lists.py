"""CPU: build.py's file lists held against csrc/ itself.  Nothing is built and no library is loaded.

source_sha() is what lets build(), bench.py and smoke() refuse a library that was not built from the tree, so a file of csrc/ it does
not read is a file whose edits go unnoticed; and an #include that does not feed its source's object key (_objects) is an edit that
leaves a stale object in the cache."""
import builtins
import os
import re

from simple_mmd_renderer_amd import build as b

QUOTED_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]+"([^"]+)"', re.M)


def _path(listed):
    return os.path.normpath(os.path.join(b.CSRC, listed))


def _includes(path):
    """The files `path` names in quoted #include lines, resolved against its own directory as the compiler does."""
    with open(path, encoding="utf-8") as f:
        return [os.path.normpath(os.path.join(os.path.dirname(path), inc)) for inc in QUOTED_INCLUDE.findall(f.read())]


def _read_by_source_sha(monkeypatch):
    read = []

    def spy(path, *args, **kwargs):
        read.append(os.path.normpath(path))
        return builtins.open(path, *args, **kwargs)

    monkeypatch.setattr(b, "open", spy, raising=False)
    b.source_sha()
    return read


def test_source_sha_reads_every_file_of_csrc(monkeypatch):
    read = _read_by_source_sha(monkeypatch)
    assert len(read) == len(set(read)), "a file is listed twice"
    assert set(read) == {_path(f) for f in b.hashed_files()}
    on_disk = {os.path.join(b.CSRC, f) for f in os.listdir(b.CSRC)}
    assert all(os.path.isfile(f) for f in on_disk), "csrc/ is flat: the lists name files, not directories"
    missing = sorted(os.path.basename(f) for f in on_disk - set(read))
    assert not missing, f"in csrc/ but not hashed by source_sha(): {missing}"


def test_every_quoted_include_is_hashed_and_keys_its_object(monkeypatch):
    hashed = set(_read_by_source_sha(monkeypatch))
    n = 0
    for f in sorted(hashed):
        for inc in _includes(f):
            n += 1
            assert inc in hashed, f"{os.path.basename(f)} includes {inc}, which source_sha() does not hash"
    assert n > 100          # the pattern finds the include lines (csrc/ has some 170)
    headers = {_path(h) for h in b.HEADERS}
    for src in b.SOURCES:
        key = {_path(f) for f in b.object_inputs(src)} | headers         # what _objects() hashes into the object's name
        assert _path(src) in key
        reached, todo = set(), [_path(src)]
        while todo:                                                      # through however many files
            for inc in _includes(todo.pop()):
                if inc not in reached:
                    reached.add(inc)
                    todo.append(inc)
        stray = sorted(os.path.basename(f) for f in reached - key)
        assert not stray, f"{src} reaches {stray}, which do not key its object: an edit there would leave the old object in use"
    # and the split of kernels.hip in particular: its pieces key the two translation units made of them, and no other
    for piece in b.KERNEL_PIECES:
        assert [s for s in b.SOURCES if piece in b.object_inputs(s)] == ["kernels.hip", "kernels_fast.hip"]
        assert piece not in b.HEADERS
