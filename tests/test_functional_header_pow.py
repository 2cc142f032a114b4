"""The headers of a HEADERS message checked whole on the device by a `-gpu=1` node: Equihash
solution, block hash and proof of work in one pass (ProcessNewBlockHeaders -> CheckBlockHeaders
-> GpuVerifyService::CheckHeaders), AcceptBlockHeader taking the hash and the verdict from it.

Node A runs `-gpu=0` (the per-header CPU path) and mines through the regtest fork. Node B
(`-gpu=1`) and node C (`-gpu=1 -gpuheaderpow=0`, the Equihash-only batch) sync A's chain and end
on its tip; B's lanes report device-computed header hashes, C's none. Every node then gets one
HEADERS message of six headers whose fourth has a valid solution and a hash above its target:
all three reject it with `high-hash` and the same misbehaviour score, after indexing the three
headers before it.
"""
import pytest

from test_header_batch_cpu import header_scenario

pytestmark = [pytest.mark.gpu, pytest.mark.functional]


def hashes_from_device(info):
    return sum(L["header_hashes"] for L in info["validation_lanes"])


def test_gpu_node_checks_header_batches_on_device(tmp_path):
    res = header_scenario(str(tmp_path), {"b": ["-gpu=1"], "c": ["-gpu=1", "-gpuheaderpow=0"]})
    (sa, ma, ta, _, fa), (sb, mb, tb, gib, fb), (sc, mc, tc, gic, fc) = res["a"], res["b"], res["c"]
    assert fa == fb == fc == 0
    assert ma == [(50, "high-hash")], ma
    assert mb == ma and mc == ma
    assert sa == sb == sc == [50]
    assert ta == tb == tc
    assert gib["enabled"] and gic["enabled"]
    # the sync's post-fork headers came in one message: B hashed them on the device, C did not
    assert hashes_from_device(gib) > 0, gib
    assert hashes_from_device(gic) == 0, gic
    assert sum(L["equihash_items"] for L in gic["validation_lanes"]) > 0, gic
