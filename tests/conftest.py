import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a ROCm GPU (MI355X) and the built HIP extension")
    config.addinivalue_line("markers", "slow: long-running CPU test")


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="session")
def adult_data_root(tmp_path_factory):
    """A data root (the layout ``fairify_amd.data.tabular`` reads) holding the UCI Adult files,
    unpacked from the gzipped copies under tests/golden/data."""
    import gzip
    import shutil

    root = tmp_path_factory.mktemp("data")
    os.makedirs(root / "adult")
    for name in ("adult.data", "adult.test"):
        with gzip.open(os.path.join(GOLDEN, "data", "adult", name + ".gz"), "rb") as src, \
                open(root / "adult" / name, "wb") as dst:
            shutil.copyfileobj(src, dst)
    return str(root)


@pytest.fixture
def adult_data(adult_data_root, monkeypatch):
    """Points the dataset loaders at the stored Adult files for one test."""
    monkeypatch.setenv("FAIRIFY_DATA", adult_data_root)
    return adult_data_root


@pytest.fixture(scope="session")
def cuda():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from fairify_amd.ops import ext

    ext()  # loud failure if the HIP extension is missing on a GPU box
    return torch.device("cuda:0")
