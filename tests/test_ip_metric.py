"""CPU tests of the inner-product metric (VROD_METRIC_IP = 2) at every layer that needs no device:
the constant agrees across the C header, the Python package and the Rust binding; the library
accepts metric 2 (and still refuses 3); the CLI creates, writes and reads back IP collections."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VROD = os.path.join(ROOT, "vrod_amd", "vrod")


def run(*args, env=None):
    return subprocess.run([VROD, *args], capture_output=True, text=True, env=env)


@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(VROD):
        subprocess.run(["make", "-C", os.path.join(ROOT, "vrod_amd", "host")], check=True)
    return VROD


def _gpu_present():
    import torch
    return torch.cuda.is_available()


def test_metric_ip_constant_agrees_everywhere():
    import vrod_amd
    from vrod_amd import index
    hdr = open(os.path.join(ROOT, "include", "vrod.h")).read()
    m = re.search(r"enum\s*\{\s*VROD_METRIC_COSINE\s*=\s*0\s*,\s*VROD_METRIC_L2\s*=\s*1\s*,\s*VROD_METRIC_IP\s*=\s*(\d+)\s*\}", hdr)
    assert m and int(m.group(1)) == 2
    assert vrod_amd.METRIC_IP == index.METRIC_IP == 2
    rs = open(os.path.join(ROOT, "bindings", "rust", "src", "lib.rs")).read()
    assert re.search(r"pub const VROD_METRIC_IP: c_int = 2;", rs)
    assert re.search(r"pub enum Metric \{[^}]*\bInnerProduct\b", rs)
    assert "Metric::InnerProduct => VROD_METRIC_IP" in rs


@pytest.mark.parametrize("name", ["ip", "IP", "dot", "inner_product"])
def test_python_metric_names(name):
    from vrod_amd import index
    assert index._enum(name, index._METRICS, "metric") == 2
    assert index._enum("cosine", index._METRICS, "metric") == 0 and index._enum("l2", index._METRICS, "metric") == 1
    with pytest.raises(ValueError):
        index._enum("manhattan", index._METRICS, "metric")


def test_index_with_ip_metric_is_not_a_bad_argument():
    import vrod_amd
    if _gpu_present():
        with vrod_amd.Index(8, "f32", "ip") as ix:
            assert ix.metric == 2 and ix.count == 0
        return
    with pytest.raises(vrod_amd.VrodError) as e:
        vrod_amd.Index(8, "f32", "ip")
    assert e.value.code == 3 and "no CPU fallback" in str(e.value)


def test_raw_create_and_merge_accept_metric_2_only():
    import vrod_amd
    L = vrod_amd.load()
    h = C.c_void_p()
    for dtype in (0, 1):
        rc = L.vrod_index_create(C.byref(h), 8, dtype, 2, None, 0)
        assert rc != 1, L.vrod_last_error()
        assert rc == (0 if _gpu_present() else 3)
        if rc == 0:
            assert L.vrod_index_destroy(h) == 0
    assert L.vrod_index_create(C.byref(h), 8, 0, 3, None, 0) == 1
    assert b"bad metric 3" in L.vrod_last_error()
    # a multi-device request is validated the same way before any device is touched
    devs = (C.c_int * 2)(0, 0)
    assert L.vrod_index_create(C.byref(h), 8, 0, 3, devs, 2) == 1
    # the merges: metric 2 passes validation (an empty merge), metric 3 does not
    for fn in (L.vrod_merge_topk_device, L.vrod_merge_topk_packed_device):
        args3 = (0, 3, None, None, 0, 0, 0, None, None, None) if fn is L.vrod_merge_topk_device else (0, 3, None, 0, 0, 0, None, None, None)
        args2 = (0, 2) + args3[2:]
        assert fn(*args3) == 1
        assert fn(*args2) != 1


def test_cli_create_metric_ip_round_trips(tmp_path, cli):
    assert run("-i", str(tmp_path), "-n", "d").returncode == 0
    db = str(tmp_path / "d")
    r = run("-d", db, "-e", "CREATE", "-a", "words metric=ip dtype=bf16")
    assert r.returncode == 0, r.stderr
    cfg = tmp_path / "d" / "words" / "vr_config"
    assert open(cfg).read().split() == ["dim=0", "metric=ip", "dtype=bf16", "count=0"]
    # a second process loads the database and lists the collection; its config is left as written
    r = run("-d", db, "-e", "LISTCOLLECTIONS")
    assert r.returncode == 0 and r.stdout.split() == ["words"]
    assert open(cfg).read().split() == ["dim=0", "metric=ip", "dtype=bf16", "count=0"]
    # other metric words keep their meaning
    assert run("-d", db, "-e", "CREATE", "-a", "a metric=l2").returncode == 0
    assert run("-d", db, "-e", "CREATE", "-a", "b metric=dot").returncode == 0
    assert open(tmp_path / "d" / "a" / "vr_config").read().split()[1] == "metric=l2"
    assert open(tmp_path / "d" / "b" / "vr_config").read().split()[1] == "metric=cosine"


def test_cli_ip_collection_without_gpu_fails_loudly_and_keeps_its_config(tmp_path, cli):
    if _gpu_present():
        pytest.skip("GPU present: tests/test_gpu_ip.py runs the collection end to end")
    assert run("-i", str(tmp_path), "-n", "d").returncode == 0
    db = str(tmp_path / "d")
    assert run("-d", db, "-e", "CREATE", "-a", "c metric=ip dtype=f32").returncode == 0
    r = run("-d", db, "-c", "c", "-e", "INSERT", "-a", "1,-2,3;x")
    assert r.returncode == 1 and "no CPU fallback" in r.stderr
    assert open(tmp_path / "d" / "c" / "vr_config").read().split() == ["dim=0", "metric=ip", "dtype=f32", "count=0"]
