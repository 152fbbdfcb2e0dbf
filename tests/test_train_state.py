"""What the trainers share (cirkit_amd/train_state.py): the layout of the device optimizer state and the flat buffers -- host
logic, on the CPU."""
import numpy as np
import torch

from cirkit_amd import _capi as capi
from cirkit_amd.train_state import DeviceOptState, FlatBuffers


def test_device_opt_state_bytes_are_the_ctypes_struct():
    st = DeviceOptState("cpu")
    assert st.counters() == (0, 0)
    st.sync(0.01, (0.9, 0.999), 1e-8, "adam")
    ref = capi.OptState(lr=0.01, b1=0.9, b2=0.999, eps=1e-8, bc1=1.0, bc2=1.0, kind=1, b1d=0.9, b2d=0.999)
    assert bytes(st.bytes.numpy()) == bytes(ref)
    assert st.skip_now_ptr - st.ptr == capi.OptState.skip_now.offset
    assert bytes(DeviceOptState("cpu").sync(0.1, (0.5, 0.6), 1e-3, "sgd").bytes.numpy()) == bytes(
        capi.OptState(lr=0.1, b1=0.5, b2=0.6, eps=1e-3, bc1=1.0, bc2=1.0, kind=0, b1d=0.5, b2d=0.6))


def test_device_opt_state_keeps_its_clock_when_the_constants_change():
    st = DeviceOptState("cpu").sync(0.01, (0.9, 0.999), 1e-8, "adam")
    dev = capi.OptState.from_buffer(st.bytes.numpy())  # (what the device's clock launches write)
    dev.step, dev.skipped, dev.skip_now, dev.bc1, dev.bc2 = 7, 2, 1, 0.5, 0.25
    assert st.counters() == (7, 2)
    ptr = st.ptr
    st.sync(0.05, (0.8, 0.99), 1e-6, "adam")
    assert st.ptr == ptr and st.counters() == (7, 2)
    ref = capi.OptState(lr=0.05, b1=0.8, b2=0.99, eps=1e-6, bc1=0.5, bc2=0.25, step=7, skipped=2, skip_now=1, kind=1, b1d=0.8, b2d=0.99)
    assert bytes(st.bytes.numpy()) == bytes(ref)


def test_flat_buffers_views_share_one_buffer_in_plan_order():
    tensors = {"a": ((2, 3), "f32"), "b": ((4,), "f32")}
    values = {"a": np.arange(6, dtype=np.float32).reshape(2, 3), "b": torch.full((4,), 7.0)}
    fb = FlatBuffers(tensors, values, "cpu", "adam")
    assert fb.param.tolist() == [0, 1, 2, 3, 4, 5, 7, 7, 7, 7]
    assert fb.store["a"].shape == (2, 3) and fb.store["b"].data_ptr() == fb.param.data_ptr() + 6 * 4
    assert fb.grads["b"].data_ptr() == fb.grad.data_ptr() + 6 * 4 and fb.grads["a"].shape == (2, 3)
    m1, m2 = fb.moments["b"]
    assert m1.data_ptr() == fb.m1.data_ptr() + 6 * 4 and m2.data_ptr() == fb.m2.data_ptr() + 6 * 4
    z = torch.zeros_like(fb.grad)
    assert fb.views(z)["b"].data_ptr() == z.data_ptr() + 6 * 4
    sgd = FlatBuffers(tensors, values, "cpu", "sgd")
    assert sgd.m1 is None and sgd.m2 is None and sgd.moments == {}
