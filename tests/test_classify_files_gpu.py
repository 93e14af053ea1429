"""The file driver of classify on the device: kspider_classify and the `classify` exe write the bytes that KSPIDER_CLASSIFY=host
writes (which tests/test_classify_files_cpu.py holds against the restatement), across batch sizes and first capacities."""
import os
import subprocess

import pytest

import classify_inputs as CI
import classify_restate as CR
from kspider_amd import engine

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, SCALED = CI.FILES_K, CI.FILES_SCALED
NAMES = ("_kSpider_classify.tsv", "_kSpider_classify_hits.tsv")


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    return CI.files_world(tmp_path_factory.mktemp("classify_files_gpu"))


def _files(prefix):
    return tuple(open(prefix + name).read() for name in NAMES)


def _run(world, monkeypatch, out, how, batch=None, first=None, min_hits=1, db=None):
    monkeypatch.setenv("KSPIDER_CLASSIFY", how)
    for name, value in (("KSPIDER_CLASSIFY_BATCH_BYTES", batch), ("KSPIDER_CLASSIFY_FIRST_CAPACITY", first)):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    prefix = str(world["dir"] / out)
    engine.classify_files(str(world["reads"]), K, SCALED, str(db or world["db"]), prefix, 2, min_hits)
    return _files(prefix)


def test_device_mode_writes_the_host_mode_bytes(world, monkeypatch):
    host = _run(world, monkeypatch, "host", "host")
    res = CR.from_kept(world["kept"], world["refs"])
    assert host == (CR.summary_tsv(world["names"], world["lengths"], res, CI.FILE_REF_NAMES), CR.hits_tsv(world["names"], res, CI.FILE_REF_NAMES, CI.REF_IDS))
    assert _run(world, monkeypatch, "device", "device") == host
    assert _run(world, monkeypatch, "b1024", "device", batch=1024) == host
    assert _run(world, monkeypatch, "bcut", "device", batch=CI.CUT) == host          # a record cut inside a repeated k-mer
    assert _run(world, monkeypatch, "cap1", "device", batch=2048, first=1) == host   # every batch overflows: compactions and regrowth
    pack = str(world["dir"] / "db.pack")
    engine.pack(str(world["db"]), K, pack, 2)
    assert _run(world, monkeypatch, "pack", "device", db=pack) == host
    m = CI.middle_hits(res["rows"])
    assert _run(world, monkeypatch, "m_device", "device", min_hits=m) == _run(world, monkeypatch, "m_host", "host", min_hits=m) != host


def test_the_exe_on_the_device(world, monkeypatch):
    host = _run(world, monkeypatch, "exe_host", "host", min_hits=2)
    exe = os.path.join(ROOT, "kspider_amd", "lib", "classify")
    prefix = str(world["dir"] / "exe")
    env = {k: v for k, v in os.environ.items() if not k.startswith("KSPIDER_CLASSIFY")}
    env.update(KSPIDER_CLASSIFY_BATCH_BYTES="4096", KSPIDER_VERBOSE="1")
    done = subprocess.run([exe, str(world["reads"]), str(K), str(SCALED), str(world["db"]), prefix, "2", "--min-hits", "2"], env=env, capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
    assert "classify:" in done.stdout and "on the host" not in done.stdout and "workgroups" in done.stdout
    assert _files(prefix) == host
