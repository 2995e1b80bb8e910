"""bench.py --dump-outputs without a GPU: dump_outputs() over stand-in resident batches writes every result field as float64,
keeps within 64 MB, draws the same seeded sample from run to run and keeps the values exact."""
import os

import numpy as np

import __graft_entry__ as graft
import bench


class FakeBatch:
    def __init__(self, res):
        self.res, self.n = res, len(res)


class FakeCtx:
    def download(self, batch):
        return batch.res.copy()


def fake_results(RESULT, n, seed):
    rng = np.random.default_rng(seed)
    raw = rng.integers(0, 256, size=n * RESULT.itemsize, dtype=np.uint8)
    return raw.view(RESULT)


def test_dump_sample_is_exact_seeded_and_bounded(tmp_path):
    RESULT = graft.load_package().host.RESULT
    sizes = (bench.DUMP_MAX_SEEDS // 2 + 3, bench.DUMP_MAX_SEEDS // 2, 1001)
    batches = [FakeBatch(fake_results(RESULT, n, k)) for k, n in enumerate(sizes)]
    whole = np.concatenate([b.res for b in batches])
    info = [bench.dump_outputs(str(tmp_path / d), FakeCtx(), batches) for d in ("a", "b")]
    assert info[0]["seeds"] == bench.DUMP_MAX_SEEDS and info[0]["of_seeds"] == len(whole)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and len(names) == 25
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64 * 1024 * 1024
    idx = np.load(tmp_path / "a" / "seed_index.npy")
    assert idx.dtype == np.float64 and (np.diff(idx) > 0).all() and idx[-1] < len(whole)
    sel = whole[idx.astype(np.int64)]
    for f in names:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b)
        if f == "seed_index.npy":
            continue
        field = f[:-4]
        side = field.split("_", 1)
        want = sel[side[0]][side[1]] if side[0] in ("left", "right") else sel[field]
        assert np.array_equal(a, want.astype(np.float64))


def test_dump_small_batch_is_whole(tmp_path):
    RESULT = graft.load_package().host.RESULT
    res = fake_results(RESULT, 777, 5)
    bench.dump_outputs(str(tmp_path), FakeCtx(), [FakeBatch(res)])
    assert np.array_equal(np.load(tmp_path / "seed_index.npy"), np.arange(777))
    assert np.array_equal(np.load(tmp_path / "left_cells.npy"), res["left"]["cells"].astype(np.float64))
