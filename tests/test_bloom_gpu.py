"""BIP37 filter membership on the GPU (K10, csrc/kernels/relay.hip bloom_match_kernel) against the
CPU oracle (CBloomFilter::contains: MurmurHash3 probes, reference src/bloom.cpp:82-91), and the
batched scan of transaction lists (csrc/net/bloomscan.cpp) with its passes on the device against
the loop of IsRelevantAndUpdate: the cases of tests/test_bloom_scan.py with ``use_gpu=True``."""
import random

import pytest

import bloom_cases
from bloom_cases import Filter, check_scan

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 7, 8, 20, 32, 33, 36, 65, 72, 73, 520, 3000]
COUNTS = [1, 63, 64, 65, 255, 256, 257, 20000]
FILTER_SIZES = [1, 2, 3, 8, 4093, 36000]
HASH_FUNCS = [1, 2, 11, 50]
TWEAKS = [0, 0xFFFFFFFF, 2147483649, 0x5BD1E995]  # the last one drawn at random once


def half_inserted(size, n_hash, tweak, elements):
    f = Filter(size, n_hash, tweak, 0)
    for e in elements[: len(elements) // 2]:
        f.insert(e)
    return bytes(f.data)


def both_ways(native, filt, n_hash, tweak, elements):
    """Device against oracle on a filter holding half the elements; the oracle says both 0 and 1."""
    want = native.bloom_contains_cpu(filt, n_hash, tweak, elements)
    assert 0 in want and 1 in want
    assert native.bloom_match_gpu(filt, n_hash, tweak, elements) == want


def test_murmur3_published_vectors(native):
    assert native.murmur3(0xFBA4C795, b"") == 0x6A396F08
    assert native.murmur3(0, bytes.fromhex("21436587")) == 0xF55B516B


def test_element_lengths_at_every_alignment(native):
    """Every tail size, the long loop past the words kept in registers, at every blob offset mod 4
    (the host path packs the elements back to back: one-byte fillers move the next one along)."""
    rng = random.Random(1)
    elements, placed, at = [], set(), 0
    for length in LENGTHS:
        for r in range(4):
            while at % 4 != r:
                elements.append(rng.randbytes(1))
                at += 1
            elements.append(rng.randbytes(length))
            placed.add((length, at % 4))
            at += length
    assert placed == {(length, r) for length in LENGTHS for r in range(4)}
    inserted = rng.sample(elements, len(elements) // 2)
    for n_hash, tweak in ((11, 7), (50, 0xFFFFFFFF)):
        f = Filter(4093, n_hash, tweak, 0)
        for e in inserted:
            f.insert(e)
        both_ways(native, bytes(f.data), n_hash, tweak, elements)


@pytest.mark.parametrize("count", COUNTS)
def test_element_counts(native, count):
    rng = random.Random(count)
    elements = [rng.randbytes(rng.choice((1, 20, 32, 33, 36, 71, 72, 73))) for _ in range(count)]
    if count == 1:  # nothing to insert and compare against: the lone element, in and out
        f = Filter(4093, 11, 3, 0)
        f.insert(b"another element")
        assert native.bloom_match_gpu(bytes(f.data), 11, 3, elements) == [0]
        f.insert(elements[0])
        assert native.bloom_match_gpu(bytes(f.data), 11, 3, elements) == [1]
        return
    both_ways(native, half_inserted(36000, 11, 3, elements), 11, 3, elements)


@pytest.mark.parametrize("size", FILTER_SIZES)
def test_filter_sizes(native, size):
    """The modulus is size * 8, no power of two for 3 and 4093 bytes. The smallest filters fill up
    with a handful of inserts, so they get few elements and hash functions, drawn until the oracle
    has both verdicts."""
    n, n_hash = (2, 1) if size <= 3 else (6, 2) if size == 8 else (300, 11)
    for seed in range(200):
        rng = random.Random(1000 * size + seed)
        elements = [rng.randbytes(rng.choice((20, 32, 33, 36))) for _ in range(n)]
        filt = half_inserted(size, n_hash, seed, elements)
        want = native.bloom_contains_cpu(filt, n_hash, seed, elements)
        if 0 in want and 1 in want:
            break
    both_ways(native, filt, n_hash, seed, elements)
    # and against many probes: 50 functions over the same filter bytes
    assert native.bloom_match_gpu(filt, 50, seed, elements) == native.bloom_contains_cpu(filt, 50, seed, elements)


@pytest.mark.parametrize("n_hash", HASH_FUNCS)
@pytest.mark.parametrize("tweak", TWEAKS)
def test_hash_functions_and_tweaks(native, n_hash, tweak):
    rng = random.Random(n_hash)
    elements = [rng.randbytes(rng.choice((20, 32, 33, 36, 72))) for _ in range(300)]
    for size in (4093, 36000):
        both_ways(native, half_inserted(size, n_hash, tweak, elements), n_hash, tweak, elements)


@pytest.mark.parametrize("j", [0, 1, 49])
def test_every_probe_is_evaluated(native, j):
    """50 functions: an inserted element with the bit of probe j alone cleared is not contained."""
    rng = random.Random(50 + j)
    elements = [rng.randbytes(33) for _ in range(64)]
    f = Filter(36000, 50, 99, 0)
    for e in elements:
        f.insert(e)
    victim = next(i for i, e in enumerate(elements) if f.bits(e).count(f.bits(e)[j]) == 1)
    bit = f.bits(elements[victim])[j]
    f.data[bit >> 3] &= ~(1 << (bit & 7))
    want = native.bloom_contains_cpu(bytes(f.data), 50, 99, elements)
    assert want[victim] == 0 and 1 in want
    assert native.bloom_match_gpu(bytes(f.data), 50, 99, elements) == want


def test_host_form_rejects_bad_arguments(native):
    ok = [b"abc"]
    for filt, n_hash, elements in ((b"", 3, ok), (b"\x01", 0, ok), (b"\x01", 51, ok), (bytes(36001), 3, ok),
                                   (b"\x01", 3, [b"abc", b""])):
        with pytest.raises(ValueError):
            native.bloom_match_gpu(filt, n_hash, 0, elements)
    assert native.bloom_match_gpu(bytes(36000), 50, 0, ok) == [0]
    assert native.bloom_match_gpu(b"\x01", 1, 0, []) == []


def test_tensor_path_equals_host_path(native):
    import torch
    from bitcoincashplus_amd import ops
    rng = random.Random(77)
    elements = [rng.randbytes(rng.choice((1, 5, 20, 33, 36, 73, 520))) for _ in range(1000)]
    filt = half_inserted(4093, 11, 2147483649, elements)
    host = ops.bloom_match(filt, 11, 2147483649, elements)
    assert host == native.bloom_contains_cpu(filt, 11, 2147483649, elements)
    offs, at = [], 0
    for e in elements:
        offs.append(at)
        at += len(e)
    whole = torch.frombuffer(bytearray(b"\0" + b"".join(elements)), dtype=torch.uint8).cuda()
    blob = whole[1:]  # the elements start at an odd device address
    assert blob.data_ptr() % 2 == 1
    offs_t = torch.tensor(offs, dtype=torch.int32, device="cuda")
    lens_t = torch.tensor([len(e) for e in elements], dtype=torch.int32, device="cuda")
    got = ops.bloom_match(filt, 11, 2147483649, (blob, offs_t, lens_t))
    assert got.is_cuda and got.dtype == torch.uint8 and got.shape == (1000,)
    assert got.cpu().tolist() == host
    # a filter tensor at an odd address as well
    fw = torch.frombuffer(bytearray(b"\0" + filt), dtype=torch.uint8).cuda()[1:]
    assert ops.bloom_match(fw, 11, 2147483649, (blob, offs_t, lens_t)).cpu().tolist() == host
    # elements the kernel must not read: empty, past the end, offset past the end
    bad_offs = torch.tensor([0, at - 2, at + 5, 3], dtype=torch.int32, device="cuda")
    bad_lens = torch.tensor([0, 3, 1, 4], dtype=torch.int32, device="cuda")
    got = ops.bloom_match(filt, 11, 2147483649, (blob, bad_offs, bad_lens)).cpu().tolist()
    assert got[:3] == [2, 2, 2] and got[3] in (0, 1)


@pytest.mark.parametrize("name", sorted(bloom_cases.cases()))
def test_scan_on_device_equals_reference_loop(native, name):
    case = bloom_cases.cases()[name]
    native.bloom_scan_reset_failures()
    before = native.bloom_scan_stats()
    info = check_scan(case["txs"], case["filter"], True, case["verdicts"], case["unchanged"])
    after = native.bloom_scan_stats()
    assert after["gpu_failures"] == before["gpu_failures"]
    if name in ("all_ones", "all_zero", "empty_vdata"):
        assert info["rounds"] == 0 and not info["used_gpu"]  # answered on the host, no device call
        return
    assert info["used_gpu"] and after["gpu_scans"] == before["gpu_scans"] + 1
    if name == "update_none":
        assert info["rounds"] == 1
    if name == "update_all_chain":
        assert info["rounds"] >= 2  # a single pre-pass would report B as 0
    if name == "random_block_few":
        assert 4 <= info["rounds"] <= 8


def test_same_transaction_effect_on_device(native):
    tries, txs, filter_ser = bloom_cases.same_transaction_case()
    assert tries is not None, "no transaction found in 1,000 tries"
    info = check_scan(txs, filter_ser, True, [True, True])
    assert info["used_gpu"]


def test_ops_bloom_scan(native):
    from bitcoincashplus_amd import ops
    case = bloom_cases.cases()["p2pubkey_only"]
    verdicts, after, info = ops.bloom_scan(case["txs"], case["filter"])
    assert verdicts == case["verdicts"] and info["used_gpu"]
    assert (verdicts, after) == native.bloom_scan_reference(case["txs"], case["filter"])
