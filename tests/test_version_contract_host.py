"""Host: ``_lib.mark_written`` -- the version contract of the library's raw-pointer writers.

A kernel that writes through ``tensor.data_ptr()`` leaves torch's version counter alone; everything keyed on ``(data_ptr, _version)``
(the kept passes and images, the tiled background, ``CameraPose``) and autograd's saved-tensor check then miss the write.  The
helper moves the counter as an in-place torch op does.  CPU tensors: the counter is host bookkeeping, no library is loaded."""
import ctypes

import pytest
import torch
from torch import nn

from opengaussian_amd._lib import mark_written


def _raw_write(t, value):
    """what a kernel does: store through the address, behind torch's back"""
    ctypes.c_float.from_address(t.data_ptr()).value = value


def test_a_raw_pointer_write_leaves_the_version_alone_and_mark_written_moves_it():
    t = torch.zeros(4)
    _raw_write(t, 3.0)
    assert float(t[0]) == 3.0 and t._version == 0          # the gap the helper closes
    mark_written(t)
    assert t._version == 1


def test_aliases_and_views_share_the_counter():
    p = nn.Parameter(torch.zeros(6))
    alias = p.detach()                                     # what train.py hands to render() from stage 1 on
    base = torch.zeros(3, 4)
    view = base[1]
    untouched, untouched_alias = torch.zeros(2), nn.Parameter(torch.zeros(2))
    before = [t._version for t in (p, alias, base, view, untouched, untouched_alias)]
    mark_written(p)
    mark_written(view)                                     # marking a view moves its base (and every other view of it)
    after = [t._version for t in (p, alias, base, view, untouched, untouched_alias)]
    assert [a - b for a, b in zip(after, before)] == [1, 1, 1, 1, 0, 0]
    mark_written(alias)                                    # ... and the other way round
    assert p._version == before[0] + 2
    assert base[2]._version == base._version               # a view made later reads the same counter


def test_none_and_empty_calls_are_accepted():
    t = torch.zeros(2)
    mark_written()
    mark_written(None)
    mark_written(None, t, None)
    assert t._version == 1


@pytest.mark.parametrize("grad_mode", [True, False], ids=["grad_on", "grad_off"])
def test_a_leaf_that_requires_grad_is_marked_in_either_grad_mode(grad_mode):
    p = nn.Parameter(torch.ones(3))
    with torch.set_grad_enabled(grad_mode):
        mark_written(p)                                    # p.add_() would raise here with grad mode on: the helper must not
        assert torch.is_grad_enabled() == grad_mode        # and leaves the caller's grad mode as it found it
    assert p._version == 1 and p.is_leaf and p.requires_grad and p.grad_fn is None


def test_marking_a_saved_tensor_makes_backward_raise_as_an_inplace_op_does():
    def run(write):
        p = nn.Parameter(torch.arange(1.0, 4.0))
        y = (p * p).sum()                                  # saves p
        write(p)
        with pytest.raises(Exception) as err:
            y.backward()
        return err

    def torch_inplace(p):
        with torch.no_grad():
            p.add_(1.0)

    def raw_then_mark(p):
        _raw_write(p, 9.0)
        mark_written(p)

    want, got = run(torch_inplace), run(raw_then_mark)
    assert got.type is want.type is RuntimeError
    assert "modified by an inplace operation" in str(want.value) and "modified by an inplace operation" in str(got.value)
    # without the mark the backward goes through, silently, over values that have since changed
    p = nn.Parameter(torch.arange(1.0, 4.0))
    y = (p * p).sum()
    _raw_write(p, 9.0)
    y.backward()
    assert torch.equal(p.grad, torch.tensor([18.0, 4.0, 6.0]))


def test_a_torch_op_on_dot_data_is_not_seen():
    """`.data` carries a version counter of its own: the documented remainder (renderer.py) besides foreign
    kernels -- `rasterizer.clear_kept()` or `mark_written(p)` after such a write."""
    p = nn.Parameter(torch.zeros(3))
    p.data.add_(1.0)
    assert p._version == 0 and float(p.detach()[0]) == 1.0
    mark_written(p)
    assert p._version == 1
