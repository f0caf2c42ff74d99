"""pmx_model_create's single upload at the shapes where a section of the device blob is empty or tiny (-m gpu): a model of one node in
one cluster, and one of two nodes without a cluster, each created, scored and destroyed, against the CPU oracle."""

import ctypes

import numpy as np
import pytest

from conftest import load_golden, rel_err
from test_gpu_parity import RTOL
from test_model_tables_cpu import hand_model

pytestmark = pytest.mark.gpu

MODELS = {
    "one_node_one_cluster": lambda: hand_model([0], [[0.0]], [[0.8]], [[0]]),
    "two_nodes_no_cluster": lambda: hand_model([0, 4], [[0.0, 4.0], [4.0, 0.0]], [[0.5, 0.7], [0.7, 0.5]], []),
}


@pytest.fixture(scope="module")
def ligands():
    """The first 8 ligands of set_6oim_c1: on the device, and as a library of their own for the oracle."""
    from pharmaconet_amd import PackedLibrary
    from pharmaconet_amd.engine import DeviceLibrary

    _, lib, _, _ = load_golden("set_6oim_c1")
    return DeviceLibrary(lib, 0), PackedLibrary.from_records([lib.record(i) for i in range(8)])


@pytest.mark.parametrize("name", tuple(MODELS))
def test_tiny_models_score_like_the_oracle(name, ligands, oracle):
    import torch

    from pharmaconet_amd import _ffi
    from pharmaconet_amd.constants import weights_vector
    from pharmaconet_amd.engine import _ModelHandle, _weights_array

    dlib, first8 = ligands
    flat = MODELS[name]()
    ref = oracle.oracle_score(flat, first8, weights_vector(None))
    mh = _ModelHandle(flat, 0)  # pmx_model_create
    scores = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda:0")
    status = torch.full((8,), -1, dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
    lib = _ffi.load()
    _ffi.check(lib.pmx_score_f64(mh.handle, dlib.handle, _weights_array(None), 0, 8, scores.data_ptr(), status.data_ptr(), ctypes.c_void_p(stream)))
    torch.cuda.synchronize()
    assert lib.pmx_model_destroy(mh.handle) == 0
    mh.handle = None
    got = scores.cpu().numpy()
    print(name, "oracle", ref.tolist(), "engine", got.tolist())
    assert np.all(status.cpu().numpy() == 0)
    zero = ref == 0
    assert np.all(got[zero] == 0.0)
    if (~zero).any():
        assert rel_err(got[~zero], ref[~zero]).max() < RTOL + 6e-8
