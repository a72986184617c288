"""CPU-only checks of rl_on_manifold_amd/build.py: the table of the seven libraries, what follows from a row's key, and the rule
that rebuilds a library for its units and what they include.  No source is edited; build_all() compiles what is stale."""
import importlib
import os

import pytest

import abi_tools as abi

CSRC_FILES = """
atacom_capi.cpp atacom_capi_common.h atacom_chart.h atacom_chart.hip atacom_chart_group.h atacom_chart_iiwa.hip
atacom_circle.hip atacom_dynamics.h atacom_dynamics_link.h atacom_envs.h atacom_evaluate.h atacom_evaluate.hip
atacom_evaluate_capi.cpp atacom_iiwa.hip atacom_iiwa_dyn.hip
atacom_iiwa_dyn_chart.hip atacom_iiwa_dyn_f64.hip atacom_iiwa_f64.hip atacom_iiwa_group.h atacom_iiwa_group.hip
atacom_iiwa_inertia.h atacom_kernels.h atacom_linalg.h atacom_mlp_host.h atacom_noise_iiwa.hip atacom_noise_iiwa_f64.hip
atacom_noise_planar.hip atacom_ops.h atacom_ops_impl.h atacom_planar.hip atacom_point.h atacom_point.hip
atacom_point_capi.cpp atacom_point_compact.h atacom_point_compact.hip atacom_point_compact_capi.cpp
atacom_point_compact_ops.h atacom_point_handle.h atacom_point_ops.h atacom_point_policy.h atacom_point_policy.hip
atacom_point_policy_capi.cpp atacom_point_policy_ops.h atacom_point_vec.h atacom_point_vec.hip atacom_point_vec_capi.cpp
atacom_point_vec_ops.h atacom_policy.h atacom_quad.h atacom_returns.h atacom_returns.hip atacom_returns_capi.cpp
""".split()
# name: (library, the variable that redirects it, directory, units); the main library's units are the rest of csrc/
TABLE = {
    'hip': ('libatacom_hip.so', 'ATACOM_LIB_OUT', 'csrc', None),
    'point': ('libatacom_point.so', 'ATACOM_POINT_LIB_OUT', 'csrc', ['atacom_point.hip', 'atacom_point_capi.cpp']),
    'point_policy': ('libatacom_point_policy.so', 'ATACOM_POINT_POLICY_LIB_OUT', 'csrc',
                     ['atacom_point_policy.hip', 'atacom_point_policy_capi.cpp']),
    'point_compact': ('libatacom_point_compact.so', 'ATACOM_POINT_COMPACT_LIB_OUT', 'csrc',
                      ['atacom_point_compact.hip', 'atacom_point_compact_capi.cpp']),
    'point_vec': ('libatacom_point_vec.so', 'ATACOM_POINT_VEC_LIB_OUT', 'csrc', ['atacom_point_vec.hip', 'atacom_point_vec_capi.cpp']),
    'returns': ('libatacom_returns.so', 'ATACOM_RETURNS_LIB_OUT', 'csrc', ['atacom_returns.hip', 'atacom_returns_capi.cpp']),
    'evaluate': ('libatacom_evaluate.so', 'ATACOM_EVALUATE_LIB_OUT', 'csrc', ['atacom_evaluate.hip', 'atacom_evaluate_capi.cpp']),
}
# the module that binds each library; the variable that redirects what it loads is the library's without _OUT
BINDINGS = {'hip': '_lib', 'point': '_lib_point', 'point_policy': '_lib_point_policy', 'point_compact': '_lib_point_compact',
            'point_vec': '_lib_point_vec', 'returns': '_lib_returns', 'evaluate': '_lib_evaluate'}
# what each later library added: its units, its private headers and its public header
OWN = {
    'point_policy': {'atacom_point_policy.hip', 'atacom_point_policy_capi.cpp', 'atacom_point_policy.h', 'atacom_point_policy_ops.h',
                     'atacom_point_policy_hip.h'},
    'point_compact': {'atacom_point_compact.hip', 'atacom_point_compact_capi.cpp', 'atacom_point_compact.h',
                      'atacom_point_compact_ops.h', 'atacom_point_compact_hip.h'},
    'point_vec': {'atacom_point_vec.hip', 'atacom_point_vec_capi.cpp', 'atacom_point_vec.h', 'atacom_point_vec_ops.h',
                  'atacom_point_vec_hip.h'},
    'returns': {'atacom_returns.h', 'atacom_returns.hip', 'atacom_returns_capi.cpp', 'atacom_returns_hip.h'},
    'evaluate': {'atacom_evaluate.h', 'atacom_evaluate.hip', 'atacom_evaluate_capi.cpp', 'atacom_evaluate_hip.h'},
}
# file: which of hip, point, point_policy, point_compact, point_vec, returns, evaluate it makes stale
STALE = {
    'atacom_capi.cpp': '1000000', 'atacom_capi_common.h': '1111111', 'atacom_linalg.h': '1111101', 'atacom_kernels.h': '1111100',
    'atacom_hip.h': '1011001', 'atacom_policy.h': '1111101', 'atacom_quad.h': '1111101',
    'atacom_iiwa_group.h': '1000000', 'atacom_ops.h': '1000000', 'atacom_ops_impl.h': '1000000', 'atacom_mlp_host.h': '1011001',
    'atacom_point.h': '0111100', 'atacom_point_handle.h': '0111100', 'atacom_point_hip.h': '0111100', 'atacom_point_ops.h': '0100000',
    'atacom_point_policy.h': '0011000', 'atacom_point_policy_ops.h': '0011000', 'atacom_point_policy_hip.h': '0011000',
    'atacom_point_policy.hip': '0010000',
    'atacom_point_compact.h': '0001000', 'atacom_point_compact_ops.h': '0001000', 'atacom_point_compact_hip.h': '0001000',
    'atacom_point_compact_capi.cpp': '0001000',
    'atacom_point_vec.h': '0000100', 'atacom_point_vec_ops.h': '0000100', 'atacom_point_vec_hip.h': '0000100',
    'atacom_point_vec.hip': '0000100', 'atacom_point_vec_capi.cpp': '0000100',
    'atacom_returns.h': '0000010', 'atacom_returns.hip': '0000010', 'atacom_returns_capi.cpp': '0000010',
    'atacom_returns_hip.h': '0000010',
    'atacom_evaluate.h': '0000001', 'atacom_evaluate.hip': '0000001', 'atacom_evaluate_capi.cpp': '0000001',
    'atacom_evaluate_hip.h': '0000001',
}


def test_the_table_is_the_six_libraries_with_their_units():
    """Seven since libatacom_evaluate.so; the test keeps the name it was given at six."""
    from rl_on_manifold_amd import build
    assert list(build.TARGETS) == list(TABLE) and len(TABLE) == 7
    for gone in ('MORE_TARGETS', 'describe', 'build_point', 'build_point_policy', 'build_point_compact', 'build_point_vec',
                 'build_returns'):
        assert not hasattr(build, gone), gone
    assert sorted(f for f in os.listdir(build.CSRC) if f.endswith(('.h', '.hip', '.cpp'))) == sorted(CSRC_FILES)
    for name, (lib, env, directory, units) in TABLE.items():
        t = build.TARGETS[name]
        assert isinstance(t, build.Target)
        assert os.path.basename(t.lib) == lib or os.environ.get(env), name
        assert t.dir == os.path.join(build.HERE, directory) == build.CSRC, name
        assert t.units == units or name == 'hip', name
        assert t.tuning == (name == 'hip')
    # the main library: every unit of csrc/ that no other library compiles, the group kernels' source first and the C ABI last
    assert build.TARGETS['hip'].units is build.UNITS and build.TARGETS['hip'].lib == build.LIB
    assert len(build.UNITS) == 14 and build.UNITS[0] == 'atacom_iiwa.hip' and build.UNITS[-1] == 'atacom_capi.cpp'
    others = [u for _, _, _, named in TABLE.values() for u in named or []]
    assert sorted(build.UNITS) == sorted(f for f in CSRC_FILES if not f.endswith('.h') and f not in others)
    units = [u for t in build.TARGETS.values() for u in t.units]
    assert len(units) == len(set(units)) == 26
    # nothing that the main library compiles names the collision-avoidance task (its kernel census is pinned,
    # tests/test_policy_kernel_resources.py)
    for f in CSRC_FILES:
        if not f.startswith('atacom_point'):
            assert 'atacom_point' not in open(os.path.join(build.CSRC, f)).read(), f


def test_what_follows_from_a_row(monkeypatch):
    """The binding module of every row loads the file that the row builds; the identity tool compares every row."""
    from rl_on_manifold_amd import build
    for name, module in BINDINGS.items():
        binding = importlib.import_module('rl_on_manifold_amd.' + module)
        lib, out_env = TABLE[name][:2]
        assert os.path.basename(binding.LIB_PATH) == lib or os.environ.get(out_env[:-len('_OUT')]), name
        if not os.environ.get(out_env) and not os.environ.get(out_env[:-len('_OUT')]):
            assert binding.LIB_PATH == build.TARGETS[name].lib == os.path.join(build.HERE, lib), name
    monkeypatch.syspath_prepend(os.path.join(abi.ROOT, 'profiles', 'tools'))
    import device_code_identity
    assert device_code_identity.LIBS == tuple(lib for lib, _, _, _ in TABLE.values()) and len(device_code_identity.LIBS) == 7


def test_a_touched_file_makes_exactly_the_libraries_that_include_it_stale(monkeypatch):
    from rl_on_manifold_amd import build
    touched = abi.fake_mtimes(monkeypatch, build)
    assert [build.stale(name) for name in build.TARGETS] == [False] * 7
    for name, want in STALE.items():
        touched[:] = [name]
        assert ''.join('01'[build.stale(n)] for n in build.TARGETS) == want, name
        assert any(os.path.exists(os.path.join(d, name)) for d in (build.CSRC, abi.INCLUDE)), name


def test_own_files_and_borrowed_headers():
    from rl_on_manifold_amd import build
    src = {name: {os.path.basename(p) for p in build.sources(t)} for name, t in build.TARGETS.items()}
    lent = {('point_policy', 'point_compact'): {'atacom_point_policy.h', 'atacom_point_policy_ops.h', 'atacom_point_policy_hip.h'}}
    for mine, own in OWN.items():
        assert own <= src[mine], mine
        for other in src:                            # editing a library's files makes no other library stale ...
            if other != mine:
                assert own & src[other] == lent.get((mine, other), set()), (mine, other)
    # ... and what a library borrows makes it stale: the handle, the environment, the policy kernel's header and validator
    assert {'atacom_point_handle.h', 'atacom_point.h', 'atacom_point_policy.h', 'atacom_point_policy_ops.h', 'atacom_policy.h',
            'atacom_point_compact_hip.h'} <= src['point_compact']
    assert {'atacom_point_handle.h', 'atacom_point.h', 'atacom_point_hip.h', 'atacom_point_vec_hip.h', 'atacom_kernels.h'} <= src['point_vec']
    assert not {'atacom_point_policy.h', 'atacom_point_policy_ops.h', 'atacom_point_compact.h', 'atacom_point_compact_ops.h'} & \
        src['point_vec']
    assert src['returns'] == OWN['returns'] | {'atacom_capi_common.h'}
    for name in src:
        assert name == 'returns' or not any('returns' in f for f in src[name]), name
    # the evaluation borrows by #include: the network, its host description and the scaffolding -- and lends nothing (above)
    assert src['evaluate'] == OWN['evaluate'] | {'atacom_policy.h', 'atacom_quad.h', 'atacom_linalg.h', 'atacom_mlp_host.h',
                                                 'atacom_capi_common.h', 'atacom_hip.h'}


def test_build_all_returns_the_seven_in_table_order():
    """Each an existing file (a library that is up to date is not compiled again)."""
    from rl_on_manifold_amd import build
    libs = build.build_all(verbose=False)
    assert libs == [t.lib for t in build.TARGETS.values()] and len(libs) == 7
    assert all(os.path.exists(p) for p in libs)


def test_the_include_closure(tmp_path):
    """sources() on files made here: no compiler and none of the repository's files."""
    from rl_on_manifold_amd import build
    (tmp_path / 'src' / 'sub').mkdir(parents=True)
    (tmp_path / 'include').mkdir()
    files = {'src/a.hip': '#include <vector>\n#include "b.h"\n  #  include "sub/c.h"\n',
             'src/b.h': '#include "../include/pub.h"\n',
             'src/sub/c.h': '#if 0\n#include "../off.h"\n#endif\n// #include "gone.h"\n',
             'src/off.h': '', 'src/unused.h': '', 'include/pub.h': '#include <stdint.h>\n', 'src/a_capi.cpp': '#include "b.h"\n'}
    for name, text in files.items():
        (tmp_path / name).write_text(text)
    target = build.Target(str(tmp_path / 'liba.so'), str(tmp_path / 'src'), ['a.hip', 'a_capi.cpp'], False)
    got = build.sources(target)
    assert got[:2] == [str(tmp_path / 'src' / u) for u in target.units]
    assert sorted(os.path.relpath(p, str(tmp_path)) for p in got) == ['include/pub.h', 'src/a.hip', 'src/a_capi.cpp', 'src/b.h',
                                                                      'src/off.h', 'src/sub/c.h']
    (tmp_path / 'src' / 'b.h').write_text('#include "missing.h"\n')
    with pytest.raises(FileNotFoundError, match=r'b\.h includes "missing\.h"'):
        build.sources(target)
