"""Host-side tests of the row state the gradient arena keeps beside its kept block (pytorch_binding/
_grads_placement.py, like_tracked): the state of the previous step is passed on only for an untouched, committed hit
of the same row size on the same stream with no foreign allocation in between; in every other case the ticket carries
a newly allocated all-zero state (or, for a plain allocation, there is no ticket). Allocator, probe and allocation
counter are the fakes of test_grads_placement.py, so this runs on CPU tensors."""
import pytest
import torch

from test_grads_placement import Fake, acts  # (puts pytorch_binding on the path)

import _grads_placement as GP  # noqa: E402


class Tracked(Fake):
    def __init__(self):
        super().__init__([7000.0, 7000.0, 7000.0])
        self.stream = 1

    def arena(self, **kw):
        return super().arena(alloc_count=lambda dev: len(self.allocs), stream_of=lambda dev: self.stream, **kw)


def step(ar, a, commit=True, mark=True, row_elems=None):
    """One backward's worth: hand-out, the 'kernel' leaves a mark in the state, commit."""
    g, tk = ar.like_tracked(a, row_elems)
    if tk is not None:
        if mark:
            tk.state[0] = 1
        if commit:
            tk.commit()
    return g, tk


def fresh(tk):
    return tk is not None and not tk.vouched and int(tk.state.sum()) == 0


def test_state_passed_on_an_untouched_committed_hit():
    f = Tracked()
    ar = f.arena()
    a = acts()
    g, t1 = step(ar, a)
    assert fresh_before_mark(t1) and t1.state.numel() == 8 and t1.state.dtype == torch.uint8
    p = g.data_ptr()
    del g
    g, t2 = step(ar, a, mark=False)
    assert g.data_ptr() == p and t2.vouched and t2.state is t1.state and int(t2.state[0]) == 1
    del g
    g, t3 = step(ar, acts(rows=4))  # fewer rows of the same size in the same block: the same state
    assert t3.vouched and t3.state is t1.state and g.shape == (4, 16)
    assert ar.track_stats == {"tickets": 3, "vouched": 2}


def fresh_before_mark(tk):
    # (step() has already marked row 0)
    return tk is not None and not tk.vouched and int(tk.state.sum()) == 1


def test_autograd_still_takes_the_gradient_without_a_copy():
    """The arena's alias is another TensorImpl on the same storage: AccumulateGrad keeps the buffer as .grad."""
    f = Tracked()
    ar = f.arena()
    x = torch.zeros(8, 16, requires_grad=True)

    class Fn(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x):
            return x.sum()

        @staticmethod
        def backward(ctx, go):
            g, tk = ar.like_tracked(x)
            ctx_ptr.append(g.data_ptr())
            tk.commit()
            return g

    ctx_ptr = []
    Fn.apply(x).backward()
    assert x.grad.data_ptr() == ctx_ptr[0]
    x.grad = None
    g, tk = ar.like_tracked(x)
    assert g.data_ptr() == ctx_ptr[0]  # reusable: the alias did not make the block look held


def test_reset_on_miss_and_after_it():
    f = Tracked()
    ar = f.arena()
    a = acts()
    g, t1 = step(ar, a)
    p = g.data_ptr()
    f.busy.add(p)
    del g
    g, t2 = step(ar, a)
    assert g.data_ptr() != p and t2 is None  # a plain block: the untracked entry
    f.on_release(g.data_ptr())
    del g
    f.busy.clear()
    g, t3 = step(ar, a, mark=False)  # the block sat in the allocator for a step: anyone may have had it
    assert g.data_ptr() == p and fresh(t3) and t3.state is not t1.state


def test_reset_when_held():
    f = Tracked()
    ar = f.arena()
    a = acts()
    g1, t1 = step(ar, a)
    g2, t2 = step(ar, a)  # g1 still held: plain
    assert t2 is None and g2.data_ptr() != g1.data_ptr()
    p = g1.data_ptr()
    del g1, g2
    g, t3 = step(ar, a, mark=False)
    assert g.data_ptr() == p and fresh(t3) and t3.state is not t1.state


def test_reset_when_uncommitted_or_untracked():
    f = Tracked()
    ar = f.arena()
    a = acts()
    g, t1 = step(ar, a, commit=False)  # an exception between hand-out and launch
    del g
    g, t2 = step(ar, a, mark=False)
    assert fresh(t2) and t2.state is not t1.state
    t2.commit()
    del g
    g = ar.like(a)  # a backward through the untracked entry
    del g
    g, t3 = step(ar, a, mark=False)
    assert fresh(t3)
    del g
    assert step(ar, a, mark=False)[1].vouched  # and tracking resumes


def _bump_grad(g):
    g.add_(1)


def _bump_view(g):
    g[2:4].zero_()


def _bump_out(g):
    torch.add(g, 1, out=g)


def _bump_no_grad(g):
    with torch.no_grad():
        g.mul_(2)


@pytest.mark.parametrize("write", [_bump_grad, _bump_view, _bump_out, _bump_no_grad], ids=lambda f: f.__name__[6:])
def test_reset_on_a_write_through_torch(write):
    f = Tracked()
    ar = f.arena()
    a = acts()
    g, t1 = step(ar, a)
    holder = g.detach()  # what autograd stores in .grad: another TensorImpl, the same version counter
    del g
    write(holder)
    del holder
    g, t2 = step(ar, a, mark=False)
    assert fresh(t2) and t2.state is not t1.state


def test_data_writes_are_the_documented_hole():
    """`.data` does not share the version counter: the write is invisible and the state is still vouched for. This
    is the hole the module docstring and INTEGRATION.md document (GP.forget() closes it by hand)."""
    f = Tracked()
    ar = f.arena()
    a = acts()
    g, t1 = step(ar, a)
    g.data.add_(1)
    del g
    g, t2 = step(ar, a, mark=False)
    assert t2.vouched
    g.data.add_(1)
    t2.commit()
    del g
    ar.forget()
    assert fresh(step(ar, a, mark=False)[1])


def test_reset_on_row_size_change():
    f = Tracked()
    ar = f.arena()
    g, t1 = step(ar, acts(rows=8, V=16))
    del g
    g, t2 = step(ar, acts(rows=16, V=8), mark=False)  # the same bytes, rows of another size
    assert fresh(t2) and t2.state.numel() == 16
    t2.commit()
    del g
    g, t3 = step(ar, acts(rows=8, V=16), mark=False, row_elems=8)  # explicit row size: the same as before
    assert t3.vouched and t3.state is t2.state


def test_reset_on_a_foreign_allocation_in_the_window():
    """Between the arena dropping the block and getting it back somebody else was served by the allocator (the
    counter moved by two): whoever that was may have been given the block, written it and freed it again."""
    f = Tracked()
    ar = f.arena()
    a = acts()
    g, t1 = step(ar, a)
    del g
    real = f.on_release

    def racing(ptr):
        real(ptr)
        f.allocs.append(-1)  # another thread's allocation

    ar._on_release = racing
    g, t2 = step(ar, a, mark=False)
    assert fresh(t2) and t2.state is not t1.state
    ar._on_release = real
    del g
    assert step(ar, a, mark=False)[1].vouched


def test_reset_on_another_stream_and_without_a_counter():
    f = Tracked()
    ar = f.arena()
    a = acts()
    g, t1 = step(ar, a)
    del g
    f.stream = 2
    g, t2 = step(ar, a, mark=False)
    assert fresh(t2) and t2.state is not t1.state
    del g
    ar._alloc_count = lambda dev: None  # the allocator cannot tell: never vouched
    assert fresh(step(ar, a, mark=False)[1])


def test_release_and_rechoose_drop_the_state():
    f = Tracked()
    ar = f.arena()
    g, t1 = step(ar, acts(rows=8))
    del g
    g, t2 = step(ar, acts(rows=32), mark=False)  # larger: a new block
    assert fresh(t2) and t2.state.numel() == 32
    t2.commit()
    del g
    ar.release()
    assert fresh(step(ar, acts(rows=32), mark=False)[1])


def test_plain_paths_have_no_ticket(monkeypatch):
    ar = GP.GradsArena(min_bytes=1 << 40, require_cuda=False)
    g, tk = ar.like_tracked(acts())
    assert tk is None and g.shape == (8, 16)
    monkeypatch.setenv("MRNNT_GRADS_PLACEMENT", "0")
    g, tk = GP.grads_tracked(acts())
    assert tk is None and g.shape == (8, 16)
