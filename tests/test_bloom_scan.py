"""The batched BIP37 scan of a transaction list (csrc/net/bloomscan.cpp) with its membership passes
on the CPU (``use_gpu=False``): verdicts and the filter afterwards must equal a loop of
CBloomFilter::IsRelevantAndUpdate (reference src/bloom.cpp:121-178), where a matching output
inserts its outpoint and later transactions match through it. tests/test_bloom_gpu.py runs the
same cases with the passes on the device."""
import pytest

import bloom_cases
from bloom_cases import check_scan


def test_murmur3_published_vectors(native):
    assert native.murmur3(0xFBA4C795, b"") == 0x6A396F08
    assert native.murmur3(0, bytes.fromhex("21436587")) == 0xF55B516B
    # and the framework's own Python implementation agrees on every tail length
    from bitcoincashplus_amd.testing.messages import CBloomFilter
    for n in range(0, 13):
        data = bytes(range(7, 7 + n))
        assert native.murmur3(0x12345678, data) == CBloomFilter.murmur3(0x12345678, data)


def test_contains_oracle_matches_inserts(native):
    f = bloom_cases.Filter(8, 3, 2147483649, 0)
    keys = [bytes([i]) * (i + 1) for i in range(12)]
    for k in keys[:3]:
        f.insert(k)
    got = native.bloom_contains_cpu(bytes(f.data), 3, 2147483649, keys)
    assert got == [int(f.contains(k)) for k in keys]
    assert got[:3] == [1, 1, 1] and 0 in got


@pytest.mark.parametrize("name", sorted(bloom_cases.cases()))
def test_scan_equals_reference_loop(name):
    case = bloom_cases.cases()[name]
    info = check_scan(case["txs"], case["filter"], False, case["verdicts"], case["unchanged"])
    assert not info["used_gpu"]
    if name == "update_none":
        assert info["rounds"] == 1
    if name == "update_all_chain":
        assert info["rounds"] >= 2  # B matches only through A's insert
    if name in ("all_ones", "all_zero", "empty_vdata"):
        assert info["rounds"] == 0  # answered without a single hash
    if name == "random_block_few":
        assert 4 <= info["rounds"] <= 8
    if name.startswith("random_block"):
        assert info["elements"] >= 3000 * 6


def test_same_transaction_effect():
    tries, txs, filter_ser = bloom_cases.same_transaction_case()
    assert tries is not None, "no transaction found in 1,000 tries"
    check_scan(txs, filter_ser, False, [True, True])


def test_fault_injection_falls_back(native):
    """A scan that starts on the "device" with the node's GPU fault injection on finishes on the
    CPU and still equals the reference."""
    case = bloom_cases.cases()["random_block_all"]
    native.bloom_scan_reset_failures()
    before = native.bloom_scan_stats()["gpu_failures"]
    native.set_gpu_fault_injection(True)
    try:
        info = check_scan(case["txs"], case["filter"], True)
    finally:
        native.set_gpu_fault_injection(False)
        native.bloom_scan_reset_failures()
    assert not info["used_gpu"] or native.bloom_scan_stats()["gpu_failures"] > before
    assert native.bloom_scan_stats()["gpu_failures"] > before


def test_use_gpu_means_the_device(native):
    """``use_gpu=True`` runs the passes on the device or raises: it never quietly stays on the CPU."""
    case = bloom_cases.cases()["update_all_chain"]
    if native.gpu_available():
        assert native.bloom_scan(case["txs"], case["filter"], True)[2]["used_gpu"]
    else:
        with pytest.raises(RuntimeError):
            native.bloom_scan(case["txs"], case["filter"], True)
