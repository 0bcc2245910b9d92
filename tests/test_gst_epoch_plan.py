"""The device-resident epoch draws its order and its rotation angles up front (gst_train.epoch_plan).  They must be the draws of the per-item
loop -- iterating DataLoader(dataset, batch_size=1, shuffle=True) and drawing theta after every item -- and leave torch's global generator
where that loop leaves it: then a run with the data on the device continues exactly like a run on the files.  CPU only."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
from torch.utils.data import DataLoader, Dataset  # noqa: E402

N = 89


class _Items(Dataset):
    """Items shaped like TrajectoriesDataset's, carrying their index."""

    def __len__(self):
        return N

    def __getitem__(self, i):
        return [torch.full((1 + i % 3, 2, 5), float(i)), torch.full((5, 1 + i % 3, 2), float(i))]


def _loop(pattern, epochs):
    """gst_train.train's loop header, verbatim: -> per epoch the (index, theta) sequence."""
    loader = DataLoader(_Items(), batch_size=1, shuffle=True, num_workers=0)
    out = []
    for _ in range(epochs):
        seq = []
        for item in loader:
            theta = None
            if pattern is not None:
                theta = (torch.randint(0, 4, ()).float() / 2. * np.pi).item() if pattern == "right_angle" else (torch.rand(()) * 2. * np.pi).item()
            seq.append((int(item[0][0, 0, 0, 0]), theta))
        out.append(seq)
    return out


@pytest.mark.parametrize("pattern", ["random", "right_angle", None])
def test_epoch_plan_reproduces_the_per_item_loops_draws(pattern):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    torch.manual_seed(1000)
    ref = _loop(pattern, 2)
    state = torch.get_rng_state()
    torch.manual_seed(1000)
    for seq in ref:
        order, thetas = T.epoch_plan(N, pattern)
        assert order.dtype == np.int64 and order.tolist() == [i for i, _ in seq] and sorted(order.tolist()) == list(range(N))
        if pattern is None:
            assert thetas is None
        else:
            assert thetas.dtype == np.float64 and thetas.tolist() == [t for _, t in seq]
    assert torch.equal(torch.get_rng_state(), state)
    if pattern == "right_angle":
        assert set(np.round(np.asarray([t for _, t in ref[0]]) / (np.pi / 2)).astype(int).tolist()) == {0, 1, 2, 3}


def test_batches_need_the_hip_backend(tmp_path):
    from crowdnav_prediction_attngraph_amd import gst_train as T
    with pytest.raises(ValueError, match="batch_size > 1"):
        T.train(str(tmp_path), str(tmp_path / "run"), batch_size=8, device="cpu")
    with pytest.raises(ValueError, match="batch_size > 1"):
        T.train(str(tmp_path), str(tmp_path / "run"), batch_size=8, backend="torch")
    with pytest.raises(ValueError, match="either a data_dir or dataset"):
        T.train(out_dir=str(tmp_path / "run"))
