"""Python front-ends for the gfx950 kernels (csrc/kernels/*.hip).

Each op runs on the MI355X and raises if no HIP device is visible — there is no
silent CPU fallback.  Ops that have a CPU implementation in the native core take
an explicit ``use_gpu=False``.

Two input paths:
* **Device-resident** (``torch.uint8`` tensors on the GPU): ``sha256d64``,
  ``short_txids``, ``bloom_match``, ``hash160``, ``wallet_match``, ``ecdsa_verify_compact`` and ``check_headers`` hand the tensors' device pointers to
  the kernels and enqueue them on the tensors' current torch stream
  (``torch.cuda.current_stream().cuda_stream``).  Results come back as GPU tensors;
  nothing is copied to the host and nothing synchronises, so the ops compose with
  other GPU work on the same stream (``gpu_api.h`` "device-resident entry points").
* **Host** (bytes, lists, CPU tensors): packed into per-device pinned staging
  buffers kept across calls (``HostBuf`` in csrc/kernels/hip_util.h), one H2D and one
  D2H DMA per call on the op's own non-blocking stream.

Kernel map (reference hot loops):
  sha256d64          K6  SHA-256d of 64-byte nodes (merkle levels)  sha256.hip
  sha256d_batch      K6  txid-style SHA-256d of variable messages   sha256.hip
  merkle_root        K6  whole-tree reduction on device              sha256.hip
  scan_nonces        K5  legacy SHA-256d header nonce scan           sha256.hip
  equihash_verify    K4  batched IsValidSolution                     equihash_verify.hip
  equihash_pow_check K5  block hash + target compare of headers      equihash_pow.hip
  check_headers      K4/K5 whole CheckBlockHeader of a header batch: solution, hash, nBits, links
                                                                     equihash_verify.hip + equihash_header.h
  equihash_mine      K1-K5 nonce states, solve, encode, hash, filter  equihash_solver.hip + equihash_pow.h
  ecdsa_verify       K8  batched secp256k1 verify                    secp256k1.hip
  verify_forkid      K8  block-path deferred checks -> verify batch  secp256k1.hip (GpuVerifyDeferred)
  short_txids        K9  BIP152 SipHash-2-4 short ids                relay.hip
  bloom_match        K10 BIP37 filter membership (MurmurHash3 probes) relay.hip
  bloom_scan         K10 a filter over a transaction list, exact     relay.hip + net/bloomscan.cpp
  hash160            K11 RIPEMD160(SHA256(m)) of byte strings         wallet_match.hip
  wallet_match       K12 txids, prevouts, scripts against the wallet's match table  wallet_match.hip
  wallet_scan        K12 a transaction list against a wallet, exact  wallet_match.hip + wallet/walletscan.cpp
  coin_select        K13 the wallet's subset search, one lane per trial  coin_select.hip + wallet/coinselect.cpp
  Equihash solving (K1-K3) is ``models.EquihashModel.gpu_solver``.
"""
from __future__ import annotations

from typing import Iterable, Sequence

from .._native import native, require_gpu

try:
    import torch
except Exception:  # pragma: no cover
    torch = None


def _on_gpu(x) -> bool:
    return torch is not None and isinstance(x, torch.Tensor) and x.is_cuda


def _u8(x, what: str):
    if x.dtype != torch.uint8:
        raise TypeError(f"{what}: expected a torch.uint8 tensor")
    return x.detach().contiguous()


def _dev_stream(t):
    """(device index, stream handle) of the current torch stream on t's device."""
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    return dev, torch.cuda.current_stream(dev).cuda_stream


def _as_bytes(x) -> bytes:
    if torch is not None and isinstance(x, torch.Tensor):
        if x.dtype != torch.uint8:
            raise TypeError("expected a torch.uint8 tensor")
        return x.detach().contiguous().cpu().numpy().tobytes()
    return bytes(x)


def sha256d64(data, device: int = -1):
    """SHA-256d of consecutive 64-byte blocks. Returns bytes, or a [N,32] uint8 tensor
    when given a tensor."""
    require_gpu("sha256d64")
    if _on_gpu(data):
        x = _u8(data, "sha256d64").view(-1)
        if x.numel() % 64:
            raise ValueError("input length must be a multiple of 64")
        n = x.numel() // 64
        out = torch.empty((n, 32), dtype=torch.uint8, device=x.device)
        dev, stream = _dev_stream(x)
        native.sha256d64_device(x.data_ptr(), out.data_ptr(), n, dev, stream)
        return out
    raw = _as_bytes(data)
    if len(raw) % 64:
        raise ValueError("input length must be a multiple of 64")
    out = native.sha256d64_batch_gpu(raw, device)
    if torch is not None and isinstance(data, torch.Tensor):
        return torch.frombuffer(bytearray(out), dtype=torch.uint8).view(-1, 32).to(data.device)
    return out


def sha256d_batch(msgs: Sequence[bytes], device: int = -1) -> list:
    require_gpu("sha256d_batch")
    return native.sha256d_batch_gpu([bytes(m) for m in msgs], device)


def merkle_root(leaves, device: int = -1):
    """Merkle root of 32-byte leaves on device. Returns (root, mutated) like the
    reference ComputeMerkleRoot (consensus/merkle.cpp)."""
    require_gpu("merkle_root")
    raw = _as_bytes(leaves) if not isinstance(leaves, (list, tuple)) else b"".join(leaves)
    if len(raw) % 32:
        raise ValueError("leaves must be 32-byte hashes")
    return native.merkle_root_gpu(raw, device)


def scan_nonces(header80: bytes, target_le: bytes, start: int, count: int, device: int = -1) -> int:
    """First nonce in [start, start+count) whose legacy header hash <= target, or -1."""
    require_gpu("scan_nonces")
    return native.sha256d_scan_nonces_gpu(bytes(header80), bytes(target_le), start, count, device)


def equihash_verify(n: int, k: int, states, solutions, device: int = -1) -> list:
    require_gpu("equihash_verify")
    return native.eh_verify_batch_gpu(n, k, list(states), [bytes(s) for s in solutions], device)


def ecdsa_verify(items: Iterable, use_gpu: bool = True, threads: int = 8):
    """Batched ECDSA verify of (pubkey, der_sig, sighash32) triples.
    Returns (list[bool], milliseconds)."""
    if use_gpu:
        require_gpu("ecdsa_verify")
    return native.ecdsa_verify_batch([(bytes(a), bytes(b), bytes(c)) for a, b, c in items], use_gpu, threads)


def equihash_pow_check(n: int, k: int, in140s, solutions, target, device: int = -1):
    """Block hashes of headers given as (140-byte Equihash input, minimal solution) pairs and
    their compare with `target` (32 bytes, little-endian 256-bit) on the device.
    Returns ([hash32], [hash <= target])."""
    require_gpu("equihash_pow_check")
    return native.eh_pow_check_gpu(n, k, [bytes(x) for x in in140s], [bytes(s) for s in solutions], bytes(target),
                                   device)


# status bits of check_headers (gpu::HeaderStatus, csrc/kernels/gpu_api.h)
HDR_SOLUTION_VALID, HDR_TARGET_LEGAL, HDR_HASH_MEETS, HDR_HASH_VALID, HDR_LINKED = 1, 2, 4, 8, 16


def check_headers(n: int, k: int, in140s, solutions, pow_limit, lenok=None, use_gpu: bool = True, device: int = -1,
                  out=None):
    """The whole of CheckBlockHeader for a batch of post-fork headers in one device pass: Equihash
    solution, block hash, nBits decode (SetCompact), target against `pow_limit` (32 bytes,
    little-endian 256-bit), hash <= target, and whether each header names the one before it.

    Host path: `in140s` is a list of 140-byte Equihash inputs and `solutions` a list of minimal
    solutions (one of another length gets HDR_HASH_VALID clear); returns ([status], [hash32]).
    ``use_gpu=False`` computes the same with the CPU consensus code.

    Device-resident path: `in140s` [cnt,140] and `solutions` [cnt, solution bytes] are
    ``torch.uint8`` GPU tensors, `lenok` an optional [cnt] uint8 tensor (0: the header's solution
    had another length); the kernels are enqueued on the current torch stream and the result is
    (status [cnt] uint8, hashes [cnt,32] uint8) on the GPU. `out` = (status, hashes) tensors of
    at least that size are written in place instead (only their first cnt rows)."""
    pow_limit = bytes(pow_limit)
    if _on_gpu(in140s):
        require_gpu("check_headers")
        if not use_gpu:
            raise ValueError("check_headers: GPU tensors with use_gpu=False")
        sw = (1 << k) * (n // (k + 1) + 1) // 8  # bytes of a minimal solution
        x, s_ = _u8(in140s, "in140s").view(-1), _u8(solutions, "solutions").view(-1)
        cnt = x.numel() // 140
        if x.numel() != cnt * 140 or s_.numel() != cnt * sw:
            raise ValueError("check_headers: in140s is [cnt,140], solutions [cnt,%d]" % sw)
        ok = torch.ones(cnt, dtype=torch.uint8, device=x.device) if lenok is None else _u8(lenok, "lenok").view(-1)
        if ok.numel() != cnt or not (x.device == s_.device == ok.device):
            raise ValueError("check_headers: lenok is [cnt]; all inputs on one device")
        if x.data_ptr() % 4:
            x = x.clone()  # the kernels read 32-bit words
        if s_.data_ptr() % 4:
            s_ = s_.clone()
        if out is None:
            status = torch.empty(cnt, dtype=torch.uint8, device=x.device)
            hashes = torch.empty((cnt, 32), dtype=torch.uint8, device=x.device)
        else:
            status, hashes = out
            if not (_on_gpu(status) and _on_gpu(hashes) and status.dtype == hashes.dtype == torch.uint8 and
                    status.is_contiguous() and hashes.is_contiguous() and status.device == hashes.device == x.device):
                raise ValueError("check_headers: out is (status, hashes), contiguous uint8 tensors on the inputs' device")
            if status.numel() < cnt or hashes.numel() < 32 * cnt or hashes.data_ptr() % 4:
                raise ValueError("check_headers: out tensors too small or hashes not 4-byte aligned")
        scratch = torch.empty(max(cnt, 1) * native.eh_check_headers_scratch_bytes(1), dtype=torch.uint8, device=x.device)
        dev, stream = _dev_stream(x)
        native.eh_check_headers_device(n, k, x.data_ptr(), s_.data_ptr(), ok.data_ptr(), pow_limit, scratch.data_ptr(),
                                       status.data_ptr(), hashes.data_ptr(), cnt, dev, stream)
        return status, hashes
    ins, sols = [bytes(a) for a in in140s], [bytes(s) for s in solutions]
    if not use_gpu:
        return native.eh_check_headers_cpu(n, k, ins, sols, pow_limit)
    require_gpu("check_headers")
    return native.eh_check_headers_gpu(n, k, ins, sols, pow_limit, device)


def equihash_mine(n: int, k: int, prefix108, nonce_first, count: int, target, batch: int = 32, device: int = 0):
    """Mine `count` nonces of a header to a target on the device: the nonces nonce_first + i
    (32 bytes or an int; 256-bit little-endian, wrapping) of the header whose 108-byte Equihash
    input is `prefix108`. Two solvers alternate over the range, each batch pipelined behind the
    other's (``after=``). Returns every hit [(nonce, solution, block hash)] in nonce order; the
    host never sees a solution above the target."""
    require_gpu("equihash_mine")
    first = nonce_first if isinstance(nonce_first, int) else int.from_bytes(bytes(nonce_first), "little")
    prefix108, target = bytes(prefix108), bytes(target)
    solvers = [native.EquihashGpuSolver(n, k, batch, device) for _ in range(2)]
    hits, pending, prev = [], [], None
    for i, off in enumerate(range(0, count, batch)):
        s = solvers[i & 1]
        if len(pending) == 2:
            hits += pending.pop(0).collect_pow()["hits"]
        nonce = ((first + off) % (1 << 256)).to_bytes(32, "little")
        s.launch_pow(prefix108, nonce, min(batch, count - off), target, after=prev)
        pending.append(s)
        prev = s
    for s in pending:
        hits += s.collect_pow()["hits"]
    return hits


__all__ = ["sha256d64", "sha256d_batch", "merkle_root", "scan_nonces", "equihash_verify", "ecdsa_verify",
           "ecdsa_verify_compact", "short_txids", "verify_forkid", "equihash_pow_check", "equihash_mine", "check_headers",
           "bloom_match", "bloom_scan", "hash160", "wallet_match", "wallet_scan", "coin_select"]


def short_txids(k0: int, k1: int, txids, device: int = -1) -> list:
    """48-bit BIP152 short ids of 32-byte txids (bytes of N*32, a list of 32-byte hashes, or a
    [N,32] uint8 tensor) under the SipHash key (k0, k1)."""
    require_gpu("short_txids")
    if _on_gpu(txids):
        x = _u8(txids, "short_txids").view(-1)
        if x.numel() % 32:
            raise ValueError("txids must be 32-byte hashes")
        if x.data_ptr() % 16:
            x = x.clone()  # the kernel reads 16-byte words
        n = x.numel() // 32
        out = torch.empty(n, dtype=torch.int64, device=x.device)  # 48-bit ids
        dev, stream = _dev_stream(x)
        native.short_txids_device(k0, k1, x.data_ptr(), out.data_ptr(), n, dev, stream)
        return out
    if isinstance(txids, (list, tuple)):
        txids = b"".join(txids)
    raw = _as_bytes(txids)
    if len(raw) % 32:
        raise ValueError("txids must be 32-byte hashes")
    return native.short_txid_batch_gpu(k0, k1, raw, device)


def ecdsa_verify_compact(msg32, sig64, pub33):
    """Batched verify of packed signatures: msg32 [N,32] digests, sig64 [N,64] compact r||s
    (low S: a high-S signature is reported invalid, as secp256k1_ecdsa_verify does), pub33
    [N,33] compressed keys. GPU tensors stay on the device and give a [N] uint8
    GPU tensor (1 = valid) on the current stream; bytes give a list of bools through the
    node's verify lanes."""
    require_gpu("ecdsa_verify_compact")
    if _on_gpu(msg32):
        m, s_, p = _u8(msg32, "msg32").view(-1), _u8(sig64, "sig64").view(-1), _u8(pub33, "pub33").view(-1)
        n = m.numel() // 32
        if m.numel() != n * 32 or s_.numel() != n * 64 or p.numel() != n * 33:
            raise ValueError("msg32/sig64/pub33 sizes")
        if not (s_.device == m.device == p.device):
            raise ValueError("inputs on different devices")
        out = torch.empty(n, dtype=torch.uint8, device=m.device)
        jobs = torch.empty(max(n, 1) * native.ecdsa_job_bytes(), dtype=torch.uint8, device=m.device)
        dev, stream = _dev_stream(m)
        native.ecdsa_verify_device(m.data_ptr(), s_.data_ptr(), p.data_ptr(), jobs.data_ptr(), out.data_ptr(), n,
                                   dev, stream)
        return out
    return native.gpu_verify_ecdsa_packed(_as_bytes(msg32), _as_bytes(sig64), _as_bytes(pub33))


def verify_forkid(items: Iterable, use_gpu: bool = True):
    """Block-path signature checks (pubkey, sig_with_hashtype, script_code, tx_bytes, n_in,
    amount) through the node's deferring checker (the digest computed as a script worker does)
    and the GPU verify batch. Returns (results, digests)."""
    if use_gpu:
        require_gpu("verify_forkid")
    return native.verify_sig_deferred(list(items), use_gpu=use_gpu)


def bloom_match(filter, n_hash: int, tweak: int, elements, device: int = -1):
    """BIP37 membership (CBloomFilter::contains) of a batch of byte strings in the filter `filter`
    (its vData, 1..36000 bytes) with `n_hash` hash functions (1..50) and tweak `tweak`.

    Host path: `filter` is bytes and `elements` a list of non-empty byte strings; returns a list
    of 0/1.

    Device-resident path: `elements` is (blob, offs, lens): a ``torch.uint8`` GPU tensor of element
    bytes at any address, and int32 GPU tensors [n] with each element's offset into it and its
    length; `filter` is bytes or a uint8 GPU tensor. The kernel is enqueued on the current torch
    stream and the result is a [n] uint8 GPU tensor: 1 / 0, and 2 for an element that is empty or
    reaches past the blob (the kernel reads nothing of it)."""
    require_gpu("bloom_match")
    if isinstance(elements, tuple) and len(elements) == 3 and _on_gpu(elements[0]):
        blob, offs, lens = elements
        blob = _u8(blob, "bloom_match").view(-1)
        if not (_on_gpu(offs) and _on_gpu(lens) and offs.dtype == lens.dtype == torch.int32):
            raise TypeError("bloom_match: offs and lens are torch.int32 GPU tensors")
        offs, lens = offs.detach().contiguous().view(-1), lens.detach().contiguous().view(-1)
        if _on_gpu(filter):
            f = _u8(filter, "bloom_match").view(-1)
        else:
            raw = _as_bytes(filter)
            if not raw:
                raise ValueError("bloom_match: empty filter")
            f = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(blob.device)
        nf = f.numel()
        n = offs.numel()
        if lens.numel() != n or not (blob.device == offs.device == lens.device == f.device):
            raise ValueError("bloom_match: offs and lens are [n]; all tensors on one device")
        out = torch.empty(n, dtype=torch.uint8, device=blob.device)
        dev, stream = _dev_stream(blob)
        native.bloom_match_device(f.data_ptr(), nf, n_hash, tweak, blob.data_ptr(), blob.numel(), offs.data_ptr(),
                                  lens.data_ptr(), out.data_ptr(), n, dev, stream)
        return out
    return native.bloom_match_gpu(_as_bytes(filter), n_hash, tweak, [bytes(e) for e in elements], device)


def bloom_scan(txs, filter_ser, use_gpu: bool = True):
    """A peer's filter over a list of serialized transactions, equal to CBloomFilter::
    IsRelevantAndUpdate on each in turn (inserts under BLOOM_UPDATE_ALL / P2PUBKEY_ONLY included),
    with the membership tests batched on the device. `filter_ser` is a ``filterload`` payload.
    Returns ([bool], the filter's payload afterwards, info) with info = {elements, rounds,
    cpu_reruns, used_gpu}. ``use_gpu=False`` runs the same batched scan on the CPU."""
    if use_gpu:
        require_gpu("bloom_scan")
    return native.bloom_scan([bytes(t) for t in txs], bytes(filter_ser), use_gpu)


def _packed_tensors(what, blob, offs, lens):
    blob = _u8(blob, what).view(-1)
    if not (_on_gpu(offs) and _on_gpu(lens) and offs.dtype == lens.dtype == torch.int32):
        raise TypeError(f"{what}: offs and lens are torch.int32 GPU tensors")
    offs, lens = offs.detach().contiguous().view(-1), lens.detach().contiguous().view(-1)
    if lens.numel() != offs.numel() or not (blob.device == offs.device == lens.device):
        raise ValueError(f"{what}: offs and lens are [n]; all tensors on one device")
    return blob, offs, lens


def hash160(messages, device: int = -1):
    """RIPEMD160(SHA256(m)) of a batch of byte strings of 0..520 bytes (CHash160).

    Host path: a list of byte strings; returns a list of 20-byte digests.

    Device-resident path: `messages` is (blob, offs, lens) as in ``bloom_match``. The kernel is
    enqueued on the current torch stream and the result is (digests [n, 20] uint8, status [n]
    uint8) on the GPU: status 1, or 2 for a message that is longer than 520 bytes or reaches past
    the blob (the kernel reads nothing of it and its digest is zero)."""
    require_gpu("hash160")
    if isinstance(messages, tuple) and len(messages) == 3 and _on_gpu(messages[0]):
        blob, offs, lens = _packed_tensors("hash160", *messages)
        n = offs.numel()
        out = torch.empty((n, 20), dtype=torch.uint8, device=blob.device)
        status = torch.empty(n, dtype=torch.uint8, device=blob.device)
        dev, stream = _dev_stream(blob)
        native.hash160_device(blob.data_ptr(), blob.numel(), offs.data_ptr(), lens.data_ptr(), out.data_ptr(),
                              status.data_ptr(), n, dev, stream)
        return out, status
    return native.hash160_gpu([bytes(m) for m in messages], device)


def wallet_match(table_desc: dict, items, device: int = -1, kind_mask: int = 7):
    """Which of `items` can concern a wallet: each item against the match table of `table_desc` =
    {salt (16 bytes, optional), keys (20-byte ids), watch (scripts), txids, spent (36-byte
    outpoints)}. An item is (kind, bytes) with kind ``native.WM_ITEM_TXID`` / ``_INPUT`` /
    ``_OUTPUT``; the result is a flag byte per item (``native.WM_HIT_K`` / ``_W`` / ``_T`` / ``_S``
    bits, ``native.WM_NOT_READ`` for an item the kernel did not read), equal to
    ``native.wallet_match_cpu``, false positives of the fingerprints included.

    Host path: `items` is a list of (kind, bytes); returns a list of ints.

    Device-resident path: `items` is (kinds, blob, offs, lens): uint8 GPU tensors of kinds [n] and
    of item bytes at any address, int32 GPU tensors [n] of offsets and lengths. The table is built
    on the host and uploaded; the kernel is enqueued on the current torch stream and the result
    is a [n] uint8 GPU tensor."""
    require_gpu("wallet_match")
    if isinstance(items, tuple) and len(items) == 4 and _on_gpu(items[0]):
        kinds = _u8(items[0], "wallet_match").view(-1)
        blob, offs, lens = _packed_tensors("wallet_match", *items[1:])
        n = offs.numel()
        if kinds.numel() != n or kinds.device != blob.device:
            raise ValueError("wallet_match: kinds is [n] on the items' device")
        t = native.wallet_match_table(table_desc)
        slots = torch.frombuffer(bytearray(t["slots"]), dtype=torch.int64).to(blob.device)
        out = torch.empty(n, dtype=torch.uint8, device=blob.device)
        dev, stream = _dev_stream(blob)
        native.wallet_match_device(slots.data_ptr(), t["n_slots"], t["k0"], t["k1"], t["has_watch"], kind_mask,
                                   kinds.data_ptr(), blob.data_ptr(), blob.numel(), offs.data_ptr(), lens.data_ptr(),
                                   out.data_ptr(), n, dev, stream)
        slots.record_stream(torch.cuda.current_stream(dev))
        return out
    return native.wallet_match_gpu(table_desc, [(int(k), bytes(b)) for k, b in items], device)


def wallet_scan(txs, wallet_desc: dict, use_gpu: bool = True, f_update: bool = True):
    """A list of serialized transactions against a wallet, equal to
    CWallet::AddToWalletIfInvolvingMe on each in turn, with the membership tests batched on the
    device. `wallet_desc` = {pubkeys, scripts (redeem scripts), watch (watch-only scripts),
    wallet_txs (serialized transactions already in the wallet)}. Returns ([bool], the wallet's
    transactions as txid || hashBlock || nIndex, its spent outpoints as outpoint || spender, info)
    with info = {items, passes, cpu_reruns, used_gpu}. ``use_gpu=False`` runs the same batched
    scan on the CPU."""
    if use_gpu:
        require_gpu("wallet_scan")
    return native.wallet_scan([bytes(t) for t in txs], wallet_desc, use_gpu, f_update)


def coin_select(values, target: int, trials: int = 1000, seed=(0, 0), both_runs: bool = False, use_gpu: bool = True,
                device: int = -1, run: int = 0, min_change: int | None = None):
    """The stochastic subset search of the wallet's coin selection (csrc/kernels/coin_select.h), one
    lane per trial: the smallest (total, trial, pass, index) with total >= `target` that `trials`
    (1..65536) trials reach over `values` (amounts > 0, sorted descending, sum below 2^63) under
    the 128-bit `seed` (k0, k1). `run` (0 or 1) picks the run's random stream. ``both_runs=True``
    searches run 0 at `target` and run 1 at `target + min_change` (the wallet's MIN_CHANGE by
    default) in one launch and returns a list of the two results.

    Host path: `values` is a list of ints or a CPU tensor; a result is (total, trial, pass, index,
    included coin indices), or None when the values sum to less than the target.
    ``use_gpu=False`` runs the CPU twin, which gives the same tuple.

    Device-resident path: `values` is a ``torch.int64`` GPU tensor. The kernels are enqueued on
    the current torch stream and the result is an int64 GPU tensor [4] (or [2, 4] with
    ``both_runs``) of (total, trial, pass, index), all -1 for no candidate; nothing synchronises
    and the amounts are not checked."""
    k0, k1 = (int(x) & 0xFFFFFFFFFFFFFFFF for x in seed)
    if min_change is None:
        min_change = native.COIN_SELECT_MIN_CHANGE
    if both_runs and run != 0:
        raise ValueError("coin_select: both_runs starts at run 0")
    targets = [int(target), int(target) + int(min_change)] if both_runs else [int(target)]
    if _on_gpu(values):
        require_gpu("coin_select")
        if not use_gpu:
            raise ValueError("coin_select: GPU tensor with use_gpu=False")
        if values.dtype != torch.int64:
            raise TypeError("coin_select: expected a torch.int64 tensor")
        x = values.detach().contiguous().view(-1)
        out = torch.empty((len(targets), 4), dtype=torch.int64, device=x.device)
        scratch = torch.empty(native.coin_select_scratch_bytes(trials, len(targets)) // 8, dtype=torch.int64,
                              device=x.device)
        dev, stream = _dev_stream(x)
        native.coin_select_device(x.data_ptr(), x.numel(), targets, run, trials, k0, k1, scratch.data_ptr(),
                                  out.data_ptr(), dev, stream)
        return out if both_runs else out[0]
    if use_gpu:
        require_gpu("coin_select")
    if torch is not None and isinstance(values, torch.Tensor):
        values = values.tolist()
    res = native.coin_select([int(v) for v in values], targets, run, trials, k0, k1, use_gpu, device)
    return list(res) if both_runs else res[0]
