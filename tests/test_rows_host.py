"""rl_on_manifold_amd/_rows.py: the host layer the learner-side modules share -- its helpers one by one, and one table that
holds every public row call of the six libraries to the same refusals in the same words.  Nothing here needs a GPU: the device
check is the last a call makes before it loads its library, so every other refusal is met on any machine."""
import ctypes as C
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

from rl_on_manifold_amd import _rows  # noqa: E402


def test_the_rules_every_tensor_of_a_call_is_held_to():
    x = torch.zeros(3, 5, 4)
    for t, name, width, words in ((torch.zeros(3, 5, 3), 'x', 4, 'shape'), (x.double(), 'action', 4, 'must be a torch.float32 tensor'),
                                  (torch.zeros(3, 5, 8)[..., ::2], 'y', 4, 'must be contiguous')):
        with pytest.raises(ValueError, match=words):
            _rows.check_rows(t, name, (3, 5), width, x)
    assert _rows.check_rows(x, 'x', (3, 5), 4, x) is x
    assert _rows.rows_of(x, 'x') == (3, 5) and _rows.rows_of(torch.zeros(4), 'x') == ()
    for bad, words in ((3.0, r'x must be a tensor \[\.\.\., n_in\]'), (torch.zeros(()), r'\[\.\.\., n_in\]'),
                       (x.half(), 'x must be float32 or float64'), (torch.zeros(3, 0, 4), 'x holds no rows')):
        with pytest.raises(ValueError, match=words):
            _rows.rows_of(bad, 'x')
    with pytest.raises(ValueError, match=r'the kernels of libatacom_fit\.so run on a GPU; got tensors on cpu'):
        _rows.needs_gpu(x, 'fit')


def test_strided_views_become_at_most_two_dimensions_per_launch():
    """_rows.launches: what is handed to the library for the shapes the modules meet."""
    launches = _rows.launches
    F = 13
    # [T, B] columns of records with a padded batch stride, next to a contiguous output
    assert launches((3, 5), [(8 * F, F), (5, 1)]) == [([0, 0], 3, 5, [(8 * F, F), (5, 1)])]
    # contiguous: one dimension
    assert launches((3, 5), [(5 * F, F), (5, 1)]) == [([0, 0], 1, 15, [(0, F), (0, 1)])]
    # [W, T, Bm] of gathered records: W and T merge
    assert launches((2, 3, 5), [(24 * F, 8 * F, F), (15, 5, 1)]) == [([0, 0], 6, 5, [(8 * F, F), (5, 1)])]
    # nothing merges: the first dimension is walked, one launch per index
    got = launches((2, 3, 5), [(100 * F, 8 * F, F), (15, 5, 1)])
    assert got == [([0, 0], 3, 5, [(8 * F, F), (5, 1)]), ([100 * F, 15], 3, 5, [(8 * F, F), (5, 1)])]
    assert launches((1, 1), [(7, 7), (1, 1)]) == [([0, 0], 1, 1, [(0, 0), (0, 0)])]
    assert launches((), [(), ()]) == [([0, 0], 1, 1, [(0, 0), (0, 0)])]


def test_one_launch_names_what_cannot_be_split():
    x = torch.zeros(2, 4, 8, 4)[:, :3, :5]
    y = torch.zeros(2, 3, 5, 1)
    with pytest.raises(ValueError, match=r'\(2, 3, 5\) of obs, target do not collapse to one \(outer, inner\) pair: a gradient cannot be split'):
        _rows.one_launch((x, y), ('obs', 'target'), (2, 3, 5), 'a gradient')
    with pytest.raises(ValueError, match=r'do not collapse to one \(outer, inner\) pair$'):
        _rows.one_launch((x,), ('obs',), (2, 3, 5))
    launch = _rows.one_launch((x[0], y[0]), ('obs', 'target'), (3, 5))
    assert launch == ([0, 0], 3, 5, [(32, 4), (5, 1)])
    assert _rows.n_rows(None, launch) == 15 and _rows.n_rows(torch.zeros(7, dtype=torch.int64), launch) == 7


def test_rows_out():
    x = torch.zeros(5, 4, dtype=torch.float64)
    t, stride = _rows.rows_out(None, 'out', 5, 1, x)
    assert t.shape == (5,) and t.dtype == x.dtype and stride == 1
    col = torch.zeros(5, 1, dtype=torch.float64)
    assert _rows.rows_out(col, 'out', 5, 1, x) == (col, 1)                   # [M, 1] is as good as [M] for width 1
    wide = torch.zeros(5, 8, dtype=torch.float64)
    assert _rows.rows_out(wide[:, 2], 'out', 5, 1, x)[1] == 8                # a strided [M]
    assert _rows.rows_out(wide[:, :3], 'eps', 5, 3, x)[1] == 8               # contiguous rows with a longer row stride
    assert _rows.rows_out(wide[:1, :3], 'eps', 1, 3, x)[1] == 3              # M = 1: the width, whatever stride(0) says
    assert _rows.rows_out(torch.zeros(1, dtype=torch.float64), 'out', 1, 1, x)[1] == 1
    assert _rows.rows_out(None, 'eps', 5, 3, x)[0].shape == (5, 3)
    for t, width, words in ((wide[:, ::2], 4, 'the 4 elements of a row of out must be contiguous'),
                            (torch.zeros(4, dtype=torch.float64), 1, r'out must be a tensor of shape \(5,\)'),
                            (torch.zeros(5, 2, dtype=torch.float64), 3, r'out must be a tensor of shape \(5, 3\)'),
                            (3.0, 1, 'out must be a tensor of shape'),
                            (torch.zeros(5), 1, 'out must be a torch.float64 tensor on cpu')):
        with pytest.raises(ValueError, match=words):
            _rows.rows_out(t, 'out', 5, width, x)


def test_optional_rows_fill_pointer_and_stride_and_join_the_list():
    class A(C.Structure):
        _fields_ = [('q_out', C.c_void_p), ('q_out_stride', C.c_int64), ('logp_out', C.c_void_p), ('logp_out_stride', C.c_int64)]
    a, x, q, seen = A(), torch.zeros(5, 4), torch.zeros(5, 8)[:, :2], []
    _rows.optional_rows(a, seen, x, 5, [('q_out', q, 2), ('logp_out', None, 1)])
    assert (a.q_out, a.q_out_stride, a.logp_out, a.logp_out_stride) == (q.data_ptr(), 8, None, 0)
    assert len(seen) == 1 and seen[0][0] is q and seen[0][1] == 'q_out'


def test_bound():
    x = torch.zeros(5, 3, dtype=torch.float64)
    assert _rows.bound(0.5, 3, x, 'low').tolist() == [0.5] * 3 and _rows.bound(0.5, 3, x, 'low').dtype == torch.float64
    assert _rows.bound([1, 2, 3], 3, x, 'low').tolist() == [1.0, 2.0, 3.0]
    assert _rows.bound(np.float32([1, 2, 3]), 3, x, 'low').is_contiguous()
    there = torch.ones(3, dtype=torch.float64)
    assert _rows.bound(there, 3, x, 'low') is there                          # used as it is
    other = _rows.bound(torch.ones(3), 3, x, 'low')                          # another dtype: converted
    assert other.dtype == torch.float64 and other.tolist() == [1.0] * 3
    assert _rows.bound(torch.ones(6, dtype=torch.float64)[::2], 3, x, 'low').is_contiguous()
    with pytest.raises(ValueError, match='high: expected a scalar or 3 values, got 2'):
        _rows.bound([1, 2], 3, x, 'high')


def test_checked_idx():
    x = torch.zeros(5, 4)
    idx = torch.tensor([4, 0, 4])
    assert _rows.checked_idx(None, x) is None and _rows.checked_idx(idx, x) is idx
    assert _rows.checked_idx(idx[:1], x).numel() == 1
    for bad, words in ((idx.int(), 'idx must be a one-dimensional int64 tensor of at least one row number'),
                       (idx[:0], 'at least one row number'), (idx.reshape(1, 3), 'one-dimensional'), ([4, 0], 'one-dimensional int64'),
                       (torch.zeros(8, dtype=torch.int64)[::2], 'idx must be contiguous and on cpu'),
                       (idx.to('meta'), 'idx must be contiguous and on cpu')):
        with pytest.raises(ValueError, match=words):
            _rows.checked_idx(bad, x)


def test_checked_blocks():
    """The union of what the modules took: whatever int() takes (fit and trust), in 0 .. the library's maximum."""
    for ok, want in ((0, 0), (1, 1), (65535, 65535), (True, 1), (False, 0), (np.int64(7), 7), (np.int32(65535), 65535), (3.0, 3)):
        got = _rows.checked_blocks(ok, 65535)
        assert got == want and type(got) is int
    for bad in (-1, 65536, np.int64(-1), np.int64(65536), None, 'many', float('nan'), float('inf')):
        with pytest.raises(ValueError, match=r'n_blocks must be 0 \(the library chooses\) or 1 \.\. 65535'):
            _rows.checked_blocks(bad, 65535)


def test_overlap_and_no_overlap():
    s = torch.zeros(64)
    a, b = s[:16], s[16:32]                                                  # touching, disjoint
    assert not _rows.overlap(a, b) and _rows.overlap(a, s[15:17]) and not _rows.overlap(a, s[:0])
    assert _rows.extent(s[4:12:2]) == (s.data_ptr() + 16, s.data_ptr() + 16 + 4 * 7)
    m = torch.zeros(6, 8)
    assert _rows.extent(m[:, 2:4].t()) == (m.data_ptr() + 4 * 2, m.data_ptr() + 4 * (5 * 8 + 4))    # a transposed column block
    _rows.no_overlap([(a, 'out')], [(b, 'obs'), (s[32:], 'action')])
    _rows.no_overlap([(a, 'out'), (b, 'action_out')], [(s[32:], 'obs')])
    _rows.no_overlap([(a, 'out.workspace'), (a, 'out.workspace')], [])      # one object under two results is not held against itself
    with pytest.raises(ValueError, match='out overlaps obs: the call does not work in place'):
        _rows.no_overlap([(a, 'out')], [(s[15:20], 'obs')])                  # one shared element
    with pytest.raises(ValueError, match='out overlaps action_out'):
        _rows.no_overlap([(a, 'out'), (s[8:24], 'action_out')], [(s[32:], 'obs')])
    with pytest.raises(ValueError, match='action_out overlaps idx'):
        _rows.no_overlap([(a, 'out'), (b, 'action_out')], _rows.inputs([s[32:48]], ['obs'], s[24:40]))
    assert _rows.inputs([a], ['obs']) == [(a, 'obs')]


def test_carve():
    class R:
        pass
    r, flat = R(), torch.arange(20.0)
    _rows.carve(r, flat, (('W', (2, 3)), ('skipped', None), ('b', (3,)), ('s', (1, 1))))
    assert r.W.shape == (2, 3) and r.b.tolist() == [6.0, 7.0, 8.0] and r.s.tolist() == [[9.0]] and r.skipped is None
    assert r.W.data_ptr() == flat.data_ptr() and r.b.data_ptr() == flat.data_ptr() + 4 * 6 and r.s.data_ptr() == flat.data_ptr() + 4 * 9


def test_reuse():
    class Out:
        def __init__(self, key, n):
            self.key, self.workspace = key, torch.empty(n, dtype=torch.uint8)
    key = (4, 2, torch.float32)
    what = lambda: "Out of a call"                                           # noqa: E731
    pair = (Out(key, 256), Out(key, 0))                                      # the first holds the workspace of a pair
    assert _rows.reuse(pair, Out, key, 256, what) is pair
    for outs, words in (((torch.zeros(3),), 'out must be the Out of a call'), ((Out((4, 3, torch.float32), 256),), 'out must be the Out'),
                        ((pair[0], 3.0), 'out must be the Out'), ((), 'out must be the Out'),
                        (pair, 'out was made for fewer workgroups: its workspace holds 256 bytes where this call needs 512')):
        with pytest.raises(ValueError, match=words):
            _rows.reuse(outs, Out, key, 512, what)


def test_network_struct():
    class S(C.Structure):
        _fields_ = [('n', C.c_int32)] + [(k, C.c_void_p) for k in ('W1', 'b1', 'shift')]

    class Net:
        pass
    net = Net()
    W1, b1 = torch.zeros(64, 4, dtype=torch.float64), torch.zeros(64)
    net.tensors = dict(W1=W1, b1=b1, shift=None)
    shapes = (('W1', (64, 4)), ('b1', (64,)), ('shift', (4,)))
    s = _rows.network_struct(net, shapes, S, 'cpu', torch.float64)
    assert s.W1 == W1.data_ptr() and s.shift is None and s.n == 0            # in place: no copy; None: a null pointer
    assert net._keep['W1'].data_ptr() == W1.data_ptr()
    assert s.b1 == net._keep['b1'].data_ptr() != b1.data_ptr() and net._keep['b1'].dtype == torch.float64   # converted, and kept
    first = net._keep
    _rows.network_struct(net, shapes, S, 'cpu', torch.float64, keep='_keep_backward')
    assert net._keep is first and net._keep_backward['W1'].data_ptr() == W1.data_ptr()
    net.tensors['shift'] = torch.zeros(5)
    with pytest.raises(ValueError, match=r'shift has the shape \(5,\) where the critic needs \(4,\)'):
        _rows.network_struct(net, shapes, S, 'cpu', torch.float64)
    net.tensors['shift'] = np.zeros(4)                                       # what torch.as_tensor takes
    assert _rows.network_struct(net, shapes, S, 'cpu', torch.float64).shift == net._keep['shift'].data_ptr()


def test_fill_sets_the_head_of_an_argument_struct():
    from rl_on_manifold_amd._lib_evaluate import View

    class A(C.Structure):
        _fields_ = [('device', C.c_int32), ('dtype', C.c_int32), ('n_blocks', C.c_int32), ('n_outer', C.c_int64), ('n_inner', C.c_int64),
                    ('obs', View), ('target', View), ('idx', C.c_void_p), ('n_idx', C.c_int64), ('workspace', C.c_void_p),
                    ('workspace_bytes', C.c_size_t), ('stream', C.c_void_p)]
    a, x, y, idx = A(), torch.zeros(3, 8, 4, dtype=torch.float64)[:, :5], torch.zeros(3, 5, 1, dtype=torch.float64), torch.tensor([1, 1])
    launch = _rows.one_launch((x, y), ('obs', 'target'), (3, 5))
    ref = types.SimpleNamespace(device=torch.device('cuda', 3), dtype=x.dtype, element_size=x.element_size)   # fill follows needs_gpu
    _rows.fill(a, ref, 7, launch, ('obs', 'target'), (x, y), idx)
    assert (a.device, a.dtype, a.n_blocks, a.n_outer, a.n_inner, a.idx, a.n_idx) == (3, _rows.DTYPES[torch.float64], 7, 3, 5, idx.data_ptr(), 2)
    assert (a.obs.ptr, a.obs.stride_outer, a.obs.stride_inner) == (x.data_ptr(), 32, 4)
    assert (a.target.ptr, a.target.stride_outer, a.target.stride_inner) == (y.data_ptr(), 5, 1)
    b = A()
    _rows.fill(b, ref, 0, launch, ('obs',), (x,))
    assert b.idx is None and b.n_idx == 0 and b.target.ptr is None


# ---------------------------------------------------------------------- the six libraries, one table
D, K = 4, 2


def _objects():
    from rl_on_manifold_amd import MlpPolicy, QCritic, SoftCritic
    lin = lambda o, i: (torch.zeros(o, i), torch.zeros(o))                  # noqa: E731
    net = lambda i, o: lin(64, i) + lin(64, 64) + lin(o, 64)                # noqa: E731
    return dict(pol=MlpPolicy(*net(D, K), std=torch.ones(K)), critic=MlpPolicy(*net(D, 1)),
                actor=MlpPolicy(*net(D, K)), q=QCritic(*lin(64, D + K), *lin(64, 64), torch.zeros(64, K), *lin(1, 64), kind='td3'),
                sac=MlpPolicy(*net(D, K), sigma_weights=net(D, K), squash=True),
                soft=[SoftCritic(*net(D + K, 1), n_act=K) for _ in range(2)])


def _calls(o):
    """{name: (call(obs, kw) -> the public call with the other row tensors shaped like obs, takes idx, out name or None)}: every
    public row call of evaluate, fit, trust, offpolicy, offgrad and soft."""
    from rl_on_manifold_amd import evaluate, fit, offgrad, offpolicy, soft, trust
    z = lambda x, *w: torch.zeros(tuple(x.shape[:-1]) + w, dtype=torch.float32)                        # noqa: E731
    M = lambda x, kw: kw['idx'].numel() if kw.get('idx') is not None else x[..., 0].numel()            # noqa: E731
    n_all = 64 * D + 64 + 4096 + 64 + 64 * K + K + K
    la = torch.zeros(1)
    return {
        'evaluate_rows': (lambda x, kw: evaluate.evaluate_rows(o['pol'], x, z(x, K), y=kw.pop('out', z(x, K)), logp=z(x), **kw), False, 'y'),
        'value_gradient': (lambda x, kw: fit.value_gradient(o['critic'], x, z(x), **kw), True, None),
        'policy_gradient': (lambda x, kw: fit.policy_gradient(o['pol'], x, z(x, K), z(x), z(x), **kw), True, None),
        'fisher_vector_product': (lambda x, kw: trust.fisher_vector_product(o['pol'], x, torch.zeros(n_all), **kw), True, None),
        'q_values': (lambda x, kw: offpolicy.q_values(o['q'], x, z(x, K), **kw), True, 'out'),
        'td_target': (lambda x, kw: offpolicy.td_target(o['actor'], o['q'], x, z(x), z(x), 0.99, **kw), True, 'out'),
        'critic_gradient': (lambda x, kw: offgrad.critic_gradient(o['q'], x, z(x, K), torch.zeros(M(x, kw)), **kw), True, None),
        'actor_gradient': (lambda x, kw: offgrad.actor_gradient(o['actor'], o['q'], x, **kw), True, None),
        'soft_td_target': (lambda x, kw: soft.soft_td_target(o['sac'], o['soft'], x, z(x), z(x), 0.99, la, torch.zeros(M(x, kw), K), **kw),
                           True, 'out'),
        'soft_critic_gradient': (lambda x, kw: soft.soft_critic_gradient(o['soft'], x, z(x, K), torch.zeros(M(x, kw)), **kw), True, None),
        'soft_actor_gradient': (lambda x, kw: soft.soft_actor_gradient(o['sac'], o['soft'], x, torch.zeros(M(x, kw), K), la, -2.0, **kw),
                                True, None),
    }


def test_every_row_call_refuses_the_common_faults_in_the_same_words(monkeypatch):
    from rl_on_manifold_amd import evaluate, fit, offgrad, offpolicy, soft, trust

    def never(*a, **k):
        raise AssertionError('the library was loaded')
    for mod, binding in ((evaluate, '_le'), (fit, '_lf'), (trust, '_lt'), (offpolicy, '_lo'), (offgrad, '_lg'), (soft, '_ls')):
        monkeypatch.setattr(getattr(mod, binding), 'load', never)
    x = torch.zeros(5, D)
    idx = torch.tensor([4, 0, 4])
    faults = [(x.half(), {}, r'(x|obs|next_obs) must be float32 or float64, got torch\.float16'),
              (torch.zeros(0, D), {}, r'(x|obs|next_obs) holds no rows: \(0, 4\)'),
              (torch.zeros(5, 2 * D)[:, ::2], {}, r'the 4 elements of a row of (x|obs|next_obs) must be contiguous \(stride 2\)'),
              (x, dict(n_blocks=-1), r'n_blocks must be 0 \(the library chooses\) or 1 \.\. 65535, got -1'),
              (x, dict(n_blocks=65536), r'n_blocks must be 0 \(the library chooses\) or 1 \.\. 65535, got 65536'),
              (x, {}, r'the kernels of libatacom_(evaluate|fit|trust|offpolicy|offgrad|soft)\.so run on a GPU; got tensors on cpu')]
    gathered = [(torch.zeros(2, 4, 8, D)[:, :3, :5], {}, r'the leading dimensions \(2, 3, 5\) of .* do not collapse to one \(outer, inner\) pair'),
                (x, dict(idx=idx.int()), 'idx must be a one-dimensional int64 tensor of at least one row number'),
                (x, dict(idx=idx[:0]), 'idx must be a one-dimensional int64 tensor of at least one row number'),
                (x, dict(idx=torch.zeros(6, dtype=torch.int64)[::2]), 'idx must be contiguous and on cpu')]
    for name, (call, takes_idx, out_name) in _calls(_objects()).items():
        for obs, kw, words in faults + (gathered if takes_idx else []):
            with pytest.raises(ValueError, match=words):
                call(obs, dict(kw))
            print('%-22s %s' % (name, words))
        if out_name:                                                         # an output that is a plain tensor, laid over the input
            store = torch.zeros(5, D + 1)
            over = store[:, D - 1:] if name == 'evaluate_rows' else store[:, D - 1]
            with pytest.raises(ValueError, match=r'%s overlaps (x|obs|next_obs): the call does not work in place' % out_name):
                call(store[:, :D], dict(out=over))
    # evaluate_rows walks what does not collapse, one launch per index: it refuses nothing there
    with pytest.raises(ValueError, match='run on a GPU'):
        _calls(_objects())['evaluate_rows'][0](torch.zeros(2, 4, 8, D)[:, :3, :5], {})


def test_soft_update_checks_its_tensors_before_the_device():
    from rl_on_manifold_amd import offpolicy
    o = _objects()
    with pytest.raises(ValueError, match='run on a GPU'):
        offpolicy.soft_update(o['q'], o['q'], 0.5)
    strided = tuple(torch.zeros(2 * t.shape[0], *t.shape[1:])[::2] for t in (o['q'].tensors[k] for k in ('W1', 'b1', 'W2', 'b2', 'W3', 'b3', 'W2a')))
    with pytest.raises(ValueError, match='contiguous, on one device and all float32 or all float64'):
        offpolicy.soft_update(strided, strided, 0.5)
