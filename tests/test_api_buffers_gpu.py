"""The device-buffer helpers of svt_av1_psyex_amd.api that the run_*_hip runners share."""
import numpy as np
import pytest

from svt_av1_psyex_amd import abi, api

pytestmark = pytest.mark.gpu


def test_arrays_come_back_as_they_went(hip_ctx):
    rng = np.random.default_rng(22)
    for a in (rng.integers(0, 256, (3, 5)).astype(np.uint8), rng.integers(0, 1 << 16, (2, 7)).astype(np.uint16)):
        t = api.to_device(a)
        assert t.is_cuda and t.element_size() == 1 and t.numel() == a.nbytes
        back = api.to_host(t, a.dtype, a.shape)
        assert back.dtype == a.dtype and np.array_equal(back, a)
        assert np.array_equal(api.to_host(t, a.dtype, count=4), a.reshape(-1)[:4])
    assert np.array_equal(api.to_host(api.to_device([[1, 2], [3, 400]], np.uint16), np.uint16, (2, 2)), [[1, 2], [3, 400]])


def test_records_come_back_as_they_went(hip_ctx):
    jobs = np.zeros(3, abi.OBMC_JOB_DTYPE)
    jobs["block"], jobs["offset"] = [7, 8, 9], [100, 2000, 30000]
    t = api.records_to_device(jobs, abi.OBMC_JOB_DTYPE)
    assert t.numel() == 3 * np.dtype(abi.OBMC_JOB_DTYPE).itemsize
    back = api.to_host(t, abi.OBMC_JOB_DTYPE)
    assert back.dtype == np.dtype(abi.OBMC_JOB_DTYPE) and np.array_equal(back, jobs)
    assert np.array_equal(api.to_host(t, abi.OBMC_JOB_DTYPE, count=2), jobs[:2])


def test_no_records_give_one_zeroed_record(hip_ctx):
    for empty in ([], np.zeros(0, abi.OBMC_JOB_DTYPE)):
        t = api.records_to_device(empty, abi.OBMC_JOB_DTYPE)
        assert np.array_equal(api.to_host(t, abi.OBMC_JOB_DTYPE), np.zeros(1, abi.OBMC_JOB_DTYPE))


def test_a_filled_tensor_has_at_least_one_byte(hip_ctx):
    t = api.filled(0, 0xA5)
    assert t.is_cuda and t.numel() == 1 and api.to_host(t).tolist() == [0xA5]
    assert api.to_host(t, np.uint16, count=0).size == 0  # what a runner reads back of an empty batch: nothing, whatever the dtype
    t = api.filled(6, 0x5A)
    assert np.array_equal(api.to_host(t, np.uint16), np.full(3, 0x5A5A, np.uint16))


def test_sample_dtype():
    assert api.sample_dtype(8) is np.uint8 and api.sample_dtype(10) is np.uint16
