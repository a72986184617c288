"""Build the package's shared libraries in-tree with hipcc for gfx950 (no GPU needed: hipcc cross-compiles).

    python -m rl_on_manifold_amd.build [--force]

TARGETS below describes each of the seven libraries: libatacom_hip.so (the air-hockey and circle tasks), libatacom_point.so (the
collision-avoidance task), libatacom_point_policy.so (its rollout with the actor network in the kernel),
libatacom_point_compact.so (that rollout in the compact record format), libatacom_point_vec.so (the task's masked step and
checkpoint), libatacom_returns.so (advantages and episode returns of a finished collection) and libatacom_evaluate.so (critic
and actor networks over the rows of a finished collection).  A library is one translation unit per group of kernels (they compile
in parallel) plus its C-ABI host file, linked into rl_on_manifold_amd/.  The .so files are git-ignored.

EXTENSIONS holds what is built beside that table, in rows of the same kind: libatacom_fit.so (the gradients of the PPO policy and
value losses, include/atacom_fit_hip.h), the eighth library.  It is not a row of TARGETS because the seven, their units, the
files directly inside csrc/ and their kernel census are pinned by the tests that guard them against accidental growth; a
library that only borrows headers by #include lives in a sub-directory of csrc/ (csrc/fit/) and in this second table, and
build(), stale() and sources() take its key like any other.  build_all() builds the seven, build_extensions() the eighth.

ADDITIONS is the third table and the open one: rows of the same kind, sources in a sub-directory of csrc/, and rows
may be appended (EXTENSIONS is pinned at its one row too).  It holds libatacom_optim.so (the Adam step with its state on the device,
include/atacom_optim_hip.h), the ninth library, and libatacom_trust.so (the Fisher-vector product of a TRPO policy step,
include/atacom_trust_hip.h), the tenth, and libatacom_offpolicy.so (the critic's Q-value, the fused TD target and the soft target
update of DDPG and TD3, include/atacom_offpolicy_hip.h), the eleventh, and libatacom_offgrad.so (the critic and actor gradients of a
DDPG / TD3 update, include/atacom_offgrad_hip.h), the twelfth, and libatacom_soft.so (the soft TD target, the critic and actor
gradients and the temperature step of a SAC update, include/atacom_soft_hip.h), the thirteenth, and libatacom_offstep.so (the Adam
step of an off-policy update with the soft update of the target networks in the same launch, include/atacom_offstep_hip.h), the
fourteenth; build_additions() builds its rows.
csrc/mlp/ is no library and has no row in any table: it holds the headers that libatacom_fit.so, libatacom_trust.so,
libatacom_offgrad.so and libatacom_soft.so share (the backward pass of the 2 x 64 network, atacom_mlp_backward.h; the host checks
of a call's views, atacom_view_checks.h, which libatacom_offpolicy.so includes too), which sources() finds through their #include
lines.

The rebuild rule: a library is stale when one of its units, or a file that they reach through `#include "..."` lines, is newer
than it.  The includes are read from the files themselves (sources()), so there is no list of headers to keep by hand.
"""
import os
import re
import subprocess
import sys
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor

from ._binding import HERE, naming

CSRC = os.path.join(HERE, 'csrc')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
ARCH = 'gfx950'
FLAGS = ['--offload-arch=' + ARCH, '-O3', '-std=c++17', '-fPIC', '-Wall', '-Wno-unused-function'] + \
    os.environ.get('ATACOM_HIPCC_FLAGS', '').split()
UNITS = ['atacom_iiwa.hip', 'atacom_iiwa_group.hip', 'atacom_iiwa_f64.hip', 'atacom_noise_iiwa.hip', 'atacom_noise_iiwa_f64.hip', 'atacom_iiwa_dyn.hip',
         'atacom_iiwa_dyn_f64.hip', 'atacom_iiwa_dyn_chart.hip', 'atacom_chart_iiwa.hip', 'atacom_planar.hip',
         'atacom_noise_planar.hip', 'atacom_chart.hip', 'atacom_circle.hip',
         'atacom_capi.cpp']           # longest first: the pool runs min(cores, units) compilers
# per-unit extra flags.  atacom_iiwa_group.hip holds the 4- / 8-lane float32 iiwa kernels alone so that they can take the
# iterative-ilp scheduler (-1.0 % on the headline step, profiles/r05_ab_sched.log) without the lane kernels of the same source
# paying for it (+29 % on the lane rollout kernel, r04_ab_sched_iterative_ilp.log; the option also crashes the compiler on
# float64 instantiations).  (-amdgpu-sched-strategy=max-ilp was tried per unit in round 1 -- planar step kernel -4 %, planar
# policy-rollout kernel +19 %, iiwa quad kernel +8 % -- and dropped, profiles/r01_lanes_vs_batch.md; round 5: +0.7 % on the headline)
# atacom_returns.hip: the fused multiply-adds of its recurrences are the explicit ones (include/atacom_returns_hip.h); the compiler
# adds none.  atacom_optim.hip: every operation of the Adam step is the individually rounded one its header writes; so are the
# target arithmetic and the soft update of atacom_offpolicy.hip (the fused multiply-adds of its float64 networks are explicit) and
# the row arithmetic of atacom_offgrad.hip (squash, its derivative, the division by act_scale, the head) and of atacom_soft.hip
# (the squashed Gaussian's sample, its log-probability and their derivatives, the target, the temperature's Adam step) and the
# Adam step and target update of atacom_offstep.hip, whose bits are those of atacom_optim.hip and of the soft update
UNIT_FLAGS = {'atacom_iiwa_group.hip': ['-mllvm', '-amdgpu-sched-strategy=iterative-ilp'],
              'atacom_returns.hip': ['-ffp-contract=off'],
              'atacom_optim.hip': ['-ffp-contract=off'],
              'atacom_offpolicy.hip': ['-ffp-contract=off'],
              'atacom_offgrad.hip': ['-ffp-contract=off'],
              'atacom_soft.hip': ['-ffp-contract=off'],
              'atacom_offstep.hip': ['-ffp-contract=off']}

# One row per library, keyed by its name: the units it compiles and `tuning`, whether it takes the ATACOM_ONLY_UNITS /
# kept-object path below.  Everything else follows from the key (_binding.naming()).  A new library is a new row here, a
# binding module with its signatures and structs, and its sources.
Target = namedtuple('Target', 'lib dir units tuning')


def _target(key, units, tuning, sub=''):
    n = naming(key)
    return Target(os.environ.get(n.env + '_OUT') or os.path.join(HERE, n.file), os.path.join(CSRC, sub) if sub else CSRC, units, tuning)


TARGETS = {key: _target(key, *row) for key, row in {
    'hip': (UNITS, True),
    # The collision-avoidance task (PointReachAtacom) is a library of its own (include/atacom_point_hip.h): its kernels stay
    # out of the main library's census and it shares only headers (the solver of atacom_linalg.h, the host scaffolding of
    # atacom_capi_common.h) with it.
    'point': (['atacom_point.hip', 'atacom_point_capi.cpp'], False),
    # The task's rollout with the actor network evaluated in the kernel (include/atacom_point_policy_hip.h): it borrows the
    # handles of libatacom_point.so (atacom_point_handle.h) and keeps the kernel census of the other two as it is.
    'point_policy': (['atacom_point_policy.hip', 'atacom_point_policy_capi.cpp'], False),
    # The task's rollout in the compact record format (include/atacom_point_compact_hip.h): it borrows the handles of
    # libatacom_point.so and the network, LDS layout and argument checks of libatacom_point_policy.so.
    'point_compact': (['atacom_point_compact.hip', 'atacom_point_compact_capi.cpp'], False),
    # The task's masked step and checkpoint (include/atacom_point_vec_hip.h): it borrows the handles and the environment
    # (atacom_point.h) of libatacom_point.so.
    'point_vec': (['atacom_point_vec.hip', 'atacom_point_vec_capi.cpp'], False),
    # The post-processing of a collection (include/atacom_returns_hip.h) belongs to no environment: it shares one header with
    # the others, the host scaffolding of atacom_capi_common.h.
    'returns': (['atacom_returns.hip', 'atacom_returns_capi.cpp'], False),
    # The network evaluation of a collection (include/atacom_evaluate_hip.h) belongs to no environment either: it borrows the
    # network of atacom_policy.h, the description of one (atacom_mlp_host.h) and the host scaffolding by #include, so the
    # kernel census of the other six stays as it is.
    'evaluate': (['atacom_evaluate.hip', 'atacom_evaluate_capi.cpp'], False),
}.items()}
LIB = TARGETS['hip'].lib

# Libraries beside the table (the module docstring says why): same rows, sources in a sub-directory of csrc/.
# The gradients of an on-policy update (include/atacom_fit_hip.h): it borrows the network of atacom_policy.h, its host
# description and the host scaffolding by `#include "../..."`, and adds no kernel or symbol to the seven.
EXTENSIONS = {
    'fit': _target('fit', ['atacom_fit.hip', 'atacom_fit_capi.cpp'], False, sub='fit'),
}


ADDITIONS = {
    'optim': _target('optim', ['atacom_optim.hip', 'atacom_optim_capi.cpp'], False, sub='optim'),
    'trust': _target('trust', ['atacom_trust.hip', 'atacom_trust_capi.cpp'], False, sub='trust'),
    'offpolicy': _target('offpolicy', ['atacom_offpolicy.hip', 'atacom_offpolicy_capi.cpp'], False, sub='offpolicy'),
    'offgrad': _target('offgrad', ['atacom_offgrad.hip', 'atacom_offgrad_capi.cpp'], False, sub='offgrad'),
    'soft': _target('soft', ['atacom_soft.hip', 'atacom_soft_capi.cpp'], False, sub='soft'),
    'offstep': _target('offstep', ['atacom_offstep.hip', 'atacom_offstep_capi.cpp'], False, sub='offstep'),
}
"""The open table: rows of the same kind as TARGETS and EXTENSIONS, and rows MAY BE APPENDED.  TARGETS and EXTENSIONS are
pinned entry by entry by the tests that guard them; this one is checked row by row (each row's own properties, and that the
table holds it), never by its length, so the next library is one more row here, a sub-directory of csrc/ and a binding module.
'optim': the Adam step of an on-policy update with its state on the device (include/atacom_optim_hip.h); it borrows the host
scaffolding by `#include "../..."` and adds no kernel or symbol to the other eight.
'trust': the Fisher-vector product of a trust-region policy step (include/atacom_trust_hip.h); it borrows the network of
atacom_policy.h, its host description, the host scaffolding and the view type of atacom_evaluate_hip.h, as 'fit' does.
'offpolicy': the forward half of a DDPG / TD3 update (include/atacom_offpolicy_hip.h); it borrows the LDS layouts of
atacom_policy.h, the host description of a network, the host scaffolding, the view type of atacom_evaluate_hip.h and the view
checks of csrc/mlp/ -- nothing else of csrc/mlp/ and nothing of 'fit', 'trust' or 'optim'.
'offgrad': the backward half of a DDPG / TD3 update (include/atacom_offgrad_hip.h); it borrows what 'offpolicy' borrows and the
backward pass of csrc/mlp/, which it shares with 'fit', 'trust' and 'soft', and declares its own critic descriptor: nothing of the
directories of 'fit', 'trust', 'optim' or 'offpolicy'.
'soft': a SAC update (include/atacom_soft_hip.h): the fused soft target, the critics' and the squashed-Gaussian actor's gradients
and Adam on log_alpha; it borrows what 'offgrad' borrows, csrc/mlp/ included, and declares its own critic descriptor: nothing of
the directories of 'fit', 'trust', 'optim', 'offpolicy' or 'offgrad'.
'offstep': the Adam step of an off-policy update with the target networks' soft update in its launch
(include/atacom_offstep_hip.h); it borrows the host scaffolding by `#include "../..."` as 'optim' does, nothing of csrc/mlp/ and
nothing of another library's directory, and lends nothing."""


def _row(name):
    for table in (TARGETS, EXTENSIONS, ADDITIONS):
        if name in table:
            return table[name]
    raise KeyError(name)

_INCLUDE = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)


def sources(target):
    """What a library is rebuilt for: its units and every file they reach through `#include "..."` lines.  The scan is textual
    (an include under a false #if, or at the start of a line of a /* */ comment, counts: that errs on the side of rebuilding,
    and such a line must name a file that exists), a name is resolved relative to the including file, and <...> includes are
    not followed.  `target` is a row or the key of one."""
    if isinstance(target, str):
        target = _row(target)
    out = [os.path.join(target.dir, u) for u in target.units]
    for path in out:                                 # grows while it is walked
        with open(path, encoding='utf-8', errors='replace') as fh:
            names = _INCLUDE.findall(fh.read())
        for name in names:
            found = os.path.normpath(os.path.join(os.path.dirname(path), name))
            if not os.path.isfile(found):
                raise FileNotFoundError('%s includes "%s", which is no file (%s)' % (path, name, found))
            if found not in out:
                out.append(found)
    return out


def stale(name):
    tg = _row(name)
    if not os.path.exists(tg.lib):
        return True
    t = os.path.getmtime(tg.lib)
    return any(os.path.getmtime(p) > t for p in sources(tg))


# kernel-tuning builds: ATACOM_KEEP_OBJ=1 keeps the objects of a build; ATACOM_ONLY_UNITS=a.hip,b.hip then recompiles only
# those units (with ATACOM_HIPCC_FLAGS applied to them alone) and links against the kept objects of the others
ONLY = [u for u in os.environ.get('ATACOM_ONLY_UNITS', '').split(',') if u]


def _compile(target, unit):
    src = os.path.join(target.dir, unit)
    tag = os.environ.get('ATACOM_OBJ_TAG', '')
    obj = os.path.join(target.dir, os.path.splitext(unit)[0] + tag + '.o')
    if ONLY and target.tuning and unit not in ONLY:
        kept = os.path.join(target.dir, os.path.splitext(unit)[0] + os.environ.get('ATACOM_BASE_TAG', '_keep') + '.o')
        if not os.path.exists(kept):
            raise RuntimeError('ATACOM_ONLY_UNITS needs the kept object %s (build once with ATACOM_KEEP_OBJ=1 ATACOM_OBJ_TAG=_keep)' % kept)
        return kept
    cmd = [HIPCC] + FLAGS + UNIT_FLAGS.get(unit, []) + (['-x', 'hip'] if unit.endswith('.cpp') else []) + ['-c', src, '-o', obj]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('hipcc failed for %s:\n%s\n%s' % (unit, ' '.join(cmd), r.stderr[-4000:]))
    return obj


# The kernels run at the edge of the register file and two compiler defects have been met there (a miscompiled float64
# instantiation in round 1; register copies under a narrowed exec mask, profiles/r06_exec_mask_copies.md).  The shipped code is
# validated with THIS compiler; another one is not refused -- tests/test_kernel_resources.py audits whatever it produced --
# but it is named.
VALIDATED_HIPCC = 'HIP version: 7.2'


def _hipcc_version():
    try:
        out = subprocess.run([HIPCC, '--version'], capture_output=True, text=True).stdout
        return next((ln.strip() for ln in out.splitlines() if ln.startswith('HIP version')), out.strip()[:60])
    except OSError as e:
        return 'unavailable (%s)' % e


def build(name='hip', force=False, verbose=True):
    """Build the library `name` of TARGETS, EXTENSIONS or ADDITIONS if it is stale (or `force`) and return its path.  The main library is fourteen units
    and a few minutes, the policy and compact rollouts about a minute each, the others a few seconds."""
    target = _row(name)
    if not force and not stale(name):
        return target.lib
    if name == 'hip':
        ver = _hipcc_version()
        if not ver.startswith(VALIDATED_HIPCC):
            print('[atacom] WARNING: building with "%s"; the kernels were validated with hipcc 7.2 -- run the code-object audits '
                  '(python -m pytest tests/test_kernel_resources.py) and the GPU suite before trusting this build' % ver, flush=True)
    if verbose:
        print('[atacom] building %s for %s ...' % (os.path.basename(target.lib), ARCH), flush=True)
    with ThreadPoolExecutor(max_workers=min(len(target.units), os.cpu_count() or 4)) as ex:
        objs = list(ex.map(lambda u: _compile(target, u), target.units))
    cmd = [HIPCC, '--offload-arch=' + ARCH, '-shared', '-fPIC', '-o', target.lib] + objs
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError('link failed:\n%s\n%s' % (' '.join(cmd), r.stderr[-4000:]))
    if not os.environ.get('ATACOM_KEEP_OBJ'):
        for o in objs:
            if not (ONLY and target.tuning and o.endswith(os.environ.get('ATACOM_BASE_TAG', '_keep') + '.o')):
                os.remove(o)
    return target.lib


def build_all(force=False, verbose=True):
    """Every library of TARGETS, in its order; their paths."""
    return [build(name, force, verbose) for name in TARGETS]


def build_extensions(force=False, verbose=True):
    """Every library of EXTENSIONS, in its order; their paths."""
    return [build(name, force, verbose) for name in EXTENSIONS]


def build_additions(force=False, verbose=True):
    """Every library of ADDITIONS, in its order; their paths."""
    return [build(name, force, verbose) for name in ADDITIONS]


if __name__ == '__main__':
    print('\n'.join(build_all(force='--force' in sys.argv) + build_extensions(force='--force' in sys.argv) +
                    build_additions(force='--force' in sys.argv)))
