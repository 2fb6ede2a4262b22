"""Where the hiprtc code cache goes: the package tree when it is
writable, else a per-user location (the tree may be read-only or
belong to another user)."""

import os

from pystella_amd.backend import hip


def test_jit_cache_env(tmp_path, monkeypatch):
    d = tmp_path / "explicit"
    monkeypatch.setenv("PYSTELLA_JIT_CACHE", str(d))
    assert hip._jit_cache_dir() == str(d)
    assert d.is_dir()


def test_jit_cache_in_tree(tmp_path, monkeypatch):
    monkeypatch.delenv("PYSTELLA_JIT_CACHE", raising=False)
    pkg = tmp_path / "pkg"
    (pkg / "backend").mkdir(parents=True)
    monkeypatch.setattr(hip, "__file__", str(pkg / "backend" / "hip.py"))
    assert hip._jit_cache_dir() == str(pkg / ".hiprtc_cache")
    assert (pkg / ".hiprtc_cache").is_dir()


def test_jit_cache_falls_back(tmp_path, monkeypatch):
    """A package tree in which no directory can be made (here: its
    path runs through a regular file, which fails for every user)."""
    monkeypatch.delenv("PYSTELLA_JIT_CACHE", raising=False)
    blocker = tmp_path / "pkg"
    blocker.write_text("")
    monkeypatch.setattr(hip, "__file__",
                        str(blocker / "backend" / "hip.py"))
    xdg = tmp_path / "xdg"
    monkeypatch.setenv("XDG_CACHE_HOME", str(xdg))
    want = xdg / "pystella_amd" / "hiprtc"
    assert hip._jit_cache_dir() == str(want)
    assert want.is_dir() and os.access(want, os.W_OK)

    # user cache unusable too -> per-user dir under the temp dir
    monkeypatch.setenv("XDG_CACHE_HOME", str(blocker / "cache"))
    monkeypatch.setenv("TMPDIR", str(tmp_path))
    import tempfile
    monkeypatch.setattr(tempfile, "tempdir", None)
    got = hip._jit_cache_dir()
    assert got == str(tmp_path / f"pystella_amd-hiprtc-{os.getuid()}")
    assert os.path.isdir(got)
