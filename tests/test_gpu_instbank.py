"""GPU checks of the instance bank extraction (csrc/instance_extract.hip): the device entry against its host twin --
``point_cluster``, ``cluster_rows``, ``counts`` and the table's integers equal, centre / radius / height equal AS BITS --
and against the numpy restatement of tools/extract_instances.py:46-76 (tests/instbank_ref.py): integers equal, doubles
within 1e-9.  That bound is derived, not measured: both sides work in double on fewer than 2 000 rows at |coord| <= 100,
below 1e-11 of summation error, and differ only in the summation order.  The fixtures are those of
test_instbank_host.py, where sklearn confirms the restatement on each of them; so a failure here is a kernel failure.
Then a cap smaller than the clusters found (guard values behind every buffer), one clumped non-lattice cloud of 20 k rows
(device against host twin only, bits), and ``InstanceBankBuilder`` on CUDA tensors up to a saved bank that drives
``TrainAugmentation.from_config`` on the device."""
import ctypes

import numpy as np
import pytest
import torch

import instbank_ref as ir
from instbank_ref import CASES, DTYPES, LABEL_DTYPES, bank_frames, check_against_ref, check_builder_instances, host, ref_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_RANDOM = {}


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def device(c, dtype=np.float64, label_dtype=np.int64, **kw):
    from openseg3d_amd import ops
    pc, cr, table, counts = ops.instance_extract(_t(c["points"].astype(dtype)), _t(c["labels"].astype(label_dtype)),
                                                 c["target_ids"], c["min_points"], c["ground_ids"], c["eps"], **kw)
    assert pc.is_cuda and cr.is_cuda and pc.dtype == cr.dtype == torch.int32
    return pc.cpu().numpy(), cr.cpu().numpy(), table, counts


def check_equal_bits(got, want):
    assert list(got[3]) == list(want[3]), (got[3], want[3])
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[2].dtype == want[2].dtype and len(got[2]) == len(want[2])
    for f in ("label", "begin", "rows", "kept"):
        assert np.array_equal(got[2][f], want[2][f]), f
    for f in ("center", "radius", "height"):
        assert got[2][f].tobytes() == want[2][f].tobytes(), f


def random_case():
    if not _RANDOM:
        c = ir.make_random()
        _RANDOM.update(case=c, host=host(c))
    return _RANDOM["case"], _RANDOM["host"]


@pytest.mark.parametrize("label_dtype", LABEL_DTYPES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_device_equals_host_twin_and_the_restatement(name, dtype, label_dtype):
    got = device(CASES[name], dtype, label_dtype)
    check_equal_bits(got, host(CASES[name], dtype, label_dtype))
    check_against_ref(got, ref_of(name))


def test_cap_smaller_than_the_clusters_found():
    from openseg3d_amd import _lib, ops
    c = CASES["sizes"]
    full = host(c)
    cap, guard = 3, 5
    pts, lab = _t(c["points"]), _t(c["labels"].astype(np.uint8))
    n = len(c["points"])
    pc = torch.full((n + guard,), -77, dtype=torch.int32, device=DEV)
    cr = torch.full((n + guard,), -77, dtype=torch.int32, device=DEV)
    table = torch.full(((cap + guard) * 7,), -1.5, dtype=torch.float64, device=DEV)
    counts = torch.full((4 + guard,), -77, dtype=torch.int32, device=DEV)
    ws = torch.empty((_lib.query("seg3d_instance_extract_workspace_bytes", n, cap),), dtype=torch.uint8, device=DEV)
    tids, mins, gids = (ctypes.c_uint8 * 3)(*c["target_ids"]), (ctypes.c_int32 * 3)(*c["min_points"]), (ctypes.c_uint8 * 5)(*c["ground_ids"])
    _lib.call("seg3d_instance_extract", pts.data_ptr(), n, 6, 8, lab.data_ptr(), 1, tids, mins, 3, gids, 5, 0.25, cap,
              pc.data_ptr(), cr.data_ptr(), table.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
              torch.cuda.current_stream().cuda_stream)
    pc, cr, table, counts = pc.cpu().numpy(), cr.cpu().numpy(), table.cpu().numpy(), counts.cpu().numpy()
    assert (pc[n:] == -77).all() and (cr[n:] == -77).all() and (counts[4:] == -77).all() and (table[cap * 7:] == -1.5).all()
    assert counts[0] == full[3][0] == 7 and counts[2] == full[3][2] and counts[3] == full[3][3]
    assert counts[1] == sum(int(k) for k in full[2]["kept"][:cap])
    assert np.array_equal(pc[:n], full[0]) and np.array_equal(cr[:n], full[1])
    assert table[:cap * 7].tobytes() == full[2][:cap].tobytes()
    old = ops.INSTANCE_EXTRACT_CAP
    try:  # the wrapper's own guess too small: one more run with the true number
        ops.INSTANCE_EXTRACT_CAP = 2
        again = device(c)
    finally:
        ops.INSTANCE_EXTRACT_CAP = old
    check_equal_bits(again, full)


@pytest.mark.parametrize("dtype", DTYPES)
def test_clumped_random_cloud_equals_host_twin(dtype):
    c, want = random_case()
    if dtype is np.float32:
        want = host(c, dtype)
    assert want[3][0] >= 40 and want[3][1] >= 10 and want[3][2] >= 5000  # many clusters, some kept, off the lattice
    got = device(c, dtype)
    check_equal_bits(got, want)
    check_equal_bits(device(c, dtype), got)  # and the same again: no dependence on the schedule


def test_builder_on_the_device_and_the_saved_bank_in_training(tmp_path):
    from openseg3d_amd import augment, config
    for dtype in DTYPES:
        b = augment.InstanceBankBuilder(label_ids=[3, 4, 10], min_points={3: 6, 4: 6, 10: 6}, eps=0.25)
        h = augment.InstanceBankBuilder(label_ids=[3, 4, 10], min_points={3: 6, 4: 6, 10: 6}, eps=0.25)
        for c in bank_frames():
            assert b.add(_t(c["points"].astype(dtype)), _t(c["labels"].astype(np.uint8))) == \
                h.add(c["points"].astype(dtype), c["labels"].astype(np.uint8))
        check_builder_instances(b.instances, dtype)
        for got, want in zip(b.instances[3], h.instances[3]):
            assert got["cluster_height"] == want["cluster_height"] and np.array_equal(got["cluster_points"], want["cluster_points"])
    path = str(tmp_path / "bank.pkl")
    b.save(path)
    cfg = config.default_cfg()
    ia = augment.InstanceAugmentation(path, instance_label_ids=[3], add_count=3)
    aug = augment.TrainAugmentation.from_config(cfg, rng="device", rng_state=np.random.RandomState(1), instance_bank=ia)
    assert aug.instance_aug is ia and np.array_equal(ia.bank.rows, b.bank().rows)
    f1, f2 = random_case()[0], CASES["snake"]  # dense ground at z = 0: there is room to paste
    p1, p2 = f1["points"].astype(np.float32), f2["points"].astype(np.float32)
    l1, l2 = f1["labels"].astype(np.uint8), f2["labels"].astype(np.uint8)
    want = aug.apply(p1, l1, None, p2, l2, None, seed=7)
    got = aug.apply(_t(p1), _t(l1), None, _t(p2), _t(l2), None, seed=7)
    for k in ("points", "point_labels", "source_rows"):
        assert got[k].is_cuda and np.array_equal(got[k].cpu().numpy(), want[k]), k
    assert len(got["instance_draw"]) == 3 and len(ia.last_decisions) == 3
    assert max(ia.last_decisions) >= 0 and (want["source_rows"] < 0).any()  # an instance of the new bank was pasted
