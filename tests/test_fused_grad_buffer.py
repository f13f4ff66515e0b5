"""The fused-gradient-buffer contract of ops._fused_grad_buffer on the CPU (no kernel runs): dq, dk and dv are recognised as ONE
[T, Hq+2Hkv, D] buffer exactly when they are its q | k | v head slices - the layout ops._TreeAttention.backward writes - and every
single departure from that layout is refused, one case per clause of the predicate.  A refusal costs a gather copy, never a wrong
number; recognising a buffer that is not one would hand a wrong gradient on, which is why each clause has its case."""
import pytest
import torch

from dynamictreeattn_amd import ops

T, Hq, Hkv, D = 3, 2, 1, 8
H3 = Hq + 2 * Hkv
BF = torch.bfloat16


def _slices(base, q_lo=0, k_lo=Hq, v_lo=Hq + Hkv):
    return base[:, q_lo:q_lo + Hq], base[:, k_lo:k_lo + Hkv], base[:, v_lo:v_lo + Hkv]


def _recognised(dq, dk, dv):
    return ops._fused_grad_buffer(dq, dk, dv, T, Hq, Hkv, D, BF)


def test_the_three_head_slices_of_one_buffer_are_recognised():
    base = torch.zeros(T, H3, D, dtype=BF)
    dq, dk, dv = _slices(base)
    assert (dq.storage_offset(), dk.storage_offset(), dv.storage_offset()) == (0, Hq * D, (Hq + Hkv) * D)
    assert _recognised(dq, dk, dv) is base


def _dv_separate():
    dq, dk, dv = _slices(torch.zeros(T, H3, D, dtype=BF))
    return dq, dk, dv.clone()


def _dq_dk_of_another_buffer():
    dq, dk, _ = _slices(torch.zeros(T, H3, D, dtype=BF))
    return dq, dk, _slices(torch.zeros(T, H3, D, dtype=BF))[2]


def _another_dtype():
    return _slices(torch.zeros(T, H3, D, dtype=torch.float16))


def _one_head_too_many():
    return _slices(torch.zeros(T, H3 + 1, D, dtype=BF))


def _transposed_base():
    base = torch.empty_strided((T, H3, D), (D, T * D, 1), dtype=BF).zero_()     # the memory of a [H3, T, D] tensor, transposed; its own base
    assert base._base is None and base.shape == (T, H3, D) and not base.is_contiguous()
    return _slices(base)


def _k_and_v_swapped():
    return _slices(torch.zeros(T, H3, D, dtype=BF), k_lo=Hq + Hkv, v_lo=Hq)


def _dq_with_a_head_stride_of_two():
    base = torch.zeros(T, H3, D, dtype=BF)
    dq = base.as_strided((T, Hq, D), (H3 * D, 2 * D, 1), 0)           # heads 0 and 2 of the same buffer
    assert dq._base is base
    return dq, _slices(base)[1], _slices(base)[2]


@pytest.mark.parametrize("case", [_dv_separate, _dq_dk_of_another_buffer, _another_dtype, _one_head_too_many, _transposed_base,
                                  _k_and_v_swapped, _dq_with_a_head_stride_of_two], ids=lambda f: f.__name__.lstrip("_"))
def test_every_departure_from_the_layout_is_refused(case):
    dq, dk, dv = case()
    assert dq.shape == (T, Hq, D) and dk.shape == dv.shape == (T, Hkv, D)
    assert _recognised(dq, dk, dv) is None


def test_the_form_without_rotation_hands_the_buffer_on_or_gathers_a_copy():
    """ops.qkv_prep_nope launches no kernel, so both of its backward paths run here: the recognised buffer comes back itself, three
    separate gradients come back gathered, with the same bits."""
    qkv = torch.randn(T, H3, D).to(BF).requires_grad_(True)
    q, k, v = ops.qkv_prep_nope(qkv, Hq, Hkv)
    assert torch.equal(q, qkv[:, :Hq]) and torch.equal(k, qkv[:, Hq:Hq + Hkv]) and torch.equal(v, qkv[:, Hq + Hkv:])
    assert q.grad_fn.saved_tensors == ()
    grads = torch.randn(T, H3, D).to(BF)
    buf = grads.clone()
    (inp,) = torch.autograd.grad([q, k, v], [qkv], list(_slices(buf)), retain_graph=True)
    assert inp.data_ptr() == buf.data_ptr()
    sep = [g.clone() for g in _slices(grads)]
    (out,) = torch.autograd.grad([q, k, v], [qkv], sep)
    assert out.data_ptr() not in [buf.data_ptr()] + [g.data_ptr() for g in sep]
    assert torch.equal(out, grads) and torch.equal(inp, grads)
