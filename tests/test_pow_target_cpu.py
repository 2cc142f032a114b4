"""Mining to a target without a device: DistributedEquihashMiner.mine_target on the CPU backend
(CPU solver + hashlib), and the device-only front end refusing to run without a GPU."""
import hashlib

import pytest

from bitcoincashplus_amd.parallel import DistributedEquihashMiner, compact_size, header_hash, nonce_bytes


def test_header_hash_layout():
    sol36, sol1344 = bytes(range(36)), bytes(i & 0xFF for i in range(1344))
    inp = bytes(range(140))
    assert compact_size(36) == b"\x24" and compact_size(68) == b"\x44" and compact_size(1344) == b"\xfd\x40\x05"
    for sol in (sol36, sol1344):
        msg = inp + compact_size(len(sol)) + sol
        assert header_hash(inp, sol) == hashlib.sha256(hashlib.sha256(msg).digest()).digest()
    assert len(inp + compact_size(1344) + sol1344) == 1487


def test_mine_target_cpu_backend(native):
    n, k = 48, 5
    prefix = bytes((i * 5 + 1) & 0xFF for i in range(108))
    # the CPU solver's own output for the first 16 nonces of this rank decides the target and the
    # number of steps, so the search cannot run dry
    found = []
    for c in range(16):
        nonce = nonce_bytes(c, 0)
        st = native.EquihashState(n, k)
        st.update(prefix + nonce)
        for s in native.eh_solve_cpu(n, k, st)[0]:
            found.append((int.from_bytes(header_hash(prefix + nonce, s), "little"), nonce, s))
    assert len(found) >= 2
    tint = sorted(h for h, _, _ in found)[len(found) // 2]
    target = tint.to_bytes(32, "little")
    miner = DistributedEquihashMiner(n, k, prefix, batch=8, backend="cpu")
    assert miner.rank == 0
    got = miner.mine_target(target, max_steps=2)
    assert got is not None
    nonce, sol = got
    assert int.from_bytes(header_hash(prefix + nonce, sol), "little") <= tint
    st = native.EquihashState(n, k)
    st.update(prefix + nonce)
    assert native.eh_is_valid_solution(n, k, st, sol)[0]
    # the first solution in search order that meets the target
    assert (nonce, sol) == next((nn, s) for h, nn, s in found if h <= tint)
    # nothing meets target 0
    assert DistributedEquihashMiner(n, k, prefix, batch=8, backend="cpu").mine_target(bytes(32), max_steps=1) is None
    with pytest.raises(ValueError):
        miner.mine_target(b"\xff" * 31)


def test_equihash_mine_needs_a_device(native, monkeypatch):
    from bitcoincashplus_amd import ops
    assert "equihash_mine" in ops.__all__ and "equihash_pow_check" in ops.__all__
    monkeypatch.setattr(native, "gpu_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.equihash_mine(48, 5, bytes(108), 0, 8, b"\xff" * 32, batch=8)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.equihash_pow_check(48, 5, [bytes(140)], [bytes(36)], b"\xff" * 32)
