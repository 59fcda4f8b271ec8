"""CPU: what the wide-row bf16 stem (64 <= 7 * Cin <= 95 under the plan option stem_bf16 = 2) fixes before it needs a
device -- the new exports, the option's three values, the weight cache and workspace of plans with it (unchanged where the narrow
kernels or the generic path serve, larger by exactly the exported size where the wide kernels do), which plans may carry bf16_states
with it, and the number of partial-sum slabs the weight gradient takes from a scratch of a given capacity."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ('simq_conv2d_fwd_stem_bf16_wide', 'simq_conv2d_fwd_stem_bf16_wide_x16', 'simq_conv2d_wgrad_stem_bf16_wide',
           'simq_conv2d_wgrad_stem_bf16_wide_x16')
NEW = ENTRIES + ('simq_conv2d_fwd_stem_bf16_wide_scratch_bytes', 'simq_conv2d_wgrad_stem_bf16_slabs')
SLOT_BYTES = 294912 * 4                      # one temporary slot of a workspace, per image: where a plan keeps the slabs


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def wcache(L, plan):
    return L._c.simq_wcache_bytes(plan.handle)


def slabs(L, B, C, cap):
    return L._c.simq_conv2d_wgrad_stem_bf16_slabs(B, 96, 96, C, ctypes.c_int64(cap))


def test_new_entry_points_are_declared_exported_and_bound(L):
    header = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'simq.h')).read(), flags=re.S)
    version_script = open(os.path.join(ROOT, 'spatial-intention-maps_amd', 'csrc', 'libsimq.map')).read()
    assert re.search(r'global:\s*simq_\*\s*;', version_script)                   # every simq_ name is exported, nothing else
    raw = ctypes.CDLL(L.LIB_PATH)
    dynamic = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dynamic.splitlines() if line.strip()}
    for name in NEW:
        proto = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, header)
        assert proto, '%s is not declared in include/simq.h' % name
        assert hasattr(raw, name) and name in exported, 'libsimq.so does not export %s' % name
        nargs = 0 if proto.group(1).strip() == 'void' else proto.group(1).count(',') + 1
        assert name in L.EXPORTS and len(L._SIGS[name][1]) == nargs, name
    # the wide entries take what the narrow entries take
    for name in ENTRIES:
        assert L._SIGS[name] == L._SIGS[name.replace('_wide', '')], name
    assert not [n for n in exported if not n.startswith('simq_')], 'the version script lets other names out'
    assert L.PlanOptions._fields_[-1][0] == 'bf16_states'                        # no new field: the option is a new VALUE of stem_bf16


def test_the_option_takes_zero_one_and_two(L):
    assert L.Plan(10, 1, 'bf16').options['stem_bf16'] == 1
    keys = set(L.Plan(10, 1, 'bf16').options)
    for v in (0, 1, 2):
        p = L.Plan(10, 1, 'bf16', options={'stem_bf16': v})
        assert p.options['stem_bf16'] == v and set(p.options) == keys
    for bad in (3, -1, 7):
        with pytest.raises(L.SimqError, match=r'stem_bf16 = %d' % bad):
            L.Plan(10, 1, 'bf16', options={'stem_bf16': bad})
        with pytest.raises(L.SimqError, match=r'stem_bf16 = %d' % bad):
            L.Plan(5, 1, 'fp32', options={'stem_bf16': bad})


def test_narrow_plans_keep_their_weight_cache_and_workspace(L):
    for cin in range(3, 10):
        a, b = L.Plan(cin, 1, 'bf16', options={'stem_bf16': 1}), L.Plan(cin, 1, 'bf16', options={'stem_bf16': 2})
        assert wcache(L, a) == wcache(L, b) > 0, cin
        for batch in (1, 5, 128):
            for fwd in (False, True):
                assert a.workspace_bytes(batch, forward_only=fwd) == b.workspace_bytes(batch, forward_only=fwd), (cin, batch, fwd)


def test_wide_plans_add_exactly_the_exported_weight_layout(L):
    wide = L._c.simq_conv2d_fwd_stem_bf16_wide_scratch_bytes()
    assert wide == 64 * (7 * 96 + 8) * 2                                         # bf16 rows of 7 x 96 + 8 elements, 64 output channels
    assert wide % 256 == 0                                                       # (the cache's slots are 256-byte aligned: nothing is lost to rounding)
    for cin in (10, 11, 12, 13):
        a, b = L.Plan(cin, 1, 'bf16', options={'stem_bf16': 1}), L.Plan(cin, 1, 'bf16', options={'stem_bf16': 2})
        assert wcache(L, b) - wcache(L, a) == wide, cin
        for batch in (1, 5, 128):
            for fwd in (False, True):
                assert a.workspace_bytes(batch, forward_only=fwd) == b.workspace_bytes(batch, forward_only=fwd), (cin, batch, fwd)
    # 7 * 14 = 98 > 95: the generic path, as with value 1; fp32 and split-bf16 plans never had the slot
    assert wcache(L, L.Plan(14, 1, 'bf16', options={'stem_bf16': 2})) == wcache(L, L.Plan(14, 1, 'bf16', options={'stem_bf16': 1}))
    for prec in ('fp32', 'bf16x3'):
        assert wcache(L, L.Plan(10, 1, prec, options={'stem_bf16': 2})) == wcache(L, L.Plan(10, 1, prec))


def test_bf16_states_with_the_wide_stem(L):
    for cin in (10, 11, 12, 13):
        a = L.Plan(cin, 1, 'bf16', options={'stem_bf16': 2})
        b = L.Plan(cin, 1, 'bf16', options={'stem_bf16': 2, 'bf16_states': 1})
        assert b.bf16_states == 1 and a.bf16_states == 0 and a.options == b.options
        assert wcache(L, a) == wcache(L, b)
        for batch in (1, 5, 128):
            for fwd in (False, True):
                wa, wb = a.workspace_bytes(batch, forward_only=fwd), b.workspace_bytes(batch, forward_only=fwd)
                assert 0 < wb <= wa, (cin, batch, fwd, wa, wb)
            # what is saved is half of the grad-mode forward's copy of the minibatch, up to the 256-byte alignment of the slots
            assert a.workspace_bytes(batch) - b.workspace_bytes(batch) >= batch * 96 * 96 * cin * 2 - 256, (cin, batch)
    # beyond the wide kernels: refused, and the message names the bound that holds under stem_bf16 = 2
    with pytest.raises(L.SimqError) as e:
        L.Plan(14, 1, 'bf16', options={'stem_bf16': 2, 'bf16_states': 1})
    msg = str(e.value)
    assert 'bf16_states' in msg and 'SIMQ_PREC_BF16' in msg and 'stem_bf16 = 1 or 2' in msg and '7 * num_input_channels <= 95' in msg, msg
    assert '14 channels' in msg, msg
    # under stem_bf16 = 1 (the default) ten channels keep today's refusal, word for word where it is asserted on
    for extra in ({}, {'stem_bf16': 1}):
        with pytest.raises(L.SimqError) as e:
            L.Plan(10, 1, 'bf16', options=dict(extra, bf16_states=1))
        msg = str(e.value)
        assert 'bf16_states' in msg and 'SIMQ_PREC_BF16' in msg and 'stem_bf16 = 1' in msg and '7 * num_input_channels <= 63' in msg, msg
        assert '95' not in msg, msg
    with pytest.raises(L.SimqError, match='bf16_states'):
        L.Plan(10, 1, 'bf16', options={'stem_bf16': 0, 'bf16_states': 1})


def test_the_slab_count_never_exceeds_the_capacity_it_is_given(L):
    for C in (10, 11, 12, 13):
        slab = 64 * 49 * C * 4
        for B in range(1, 131):
            want = min(512, 9 * B)                                               # what the batch asks for: ceil(72 B / 8) blocks, 512 at most
            assert slabs(L, B, C, -1) == want
            got = slabs(L, B, C, B * SLOT_BYTES)
            assert 1 <= got <= want and got * slab <= B * SLOT_BYTES, (C, B, got)
            assert got == min(want, B * SLOT_BYTES // slab), (C, B, got)           # ... and no fewer than fit
    # the case the walk would have overrun: one image of 13 channels asks for 9 slabs of 163 072 bytes, the slot holds 7
    assert slabs(L, 1, 13, SLOT_BYTES) == 7 and slabs(L, 1, 11, SLOT_BYTES) == 8 and slabs(L, 1, 10, SLOT_BYTES) == 9
    # narrow plans: a slot holds what the batch asks for, so they launch the grid they launched
    for C in range(1, 10):
        for B in list(range(1, 131)) + [512, 1000]:
            assert slabs(L, B, C, B * SLOT_BYTES) == slabs(L, B, C, -1) == min(512, 9 * B), (C, B)
    # capacities around one slab, and bad arguments
    one = 64 * 49 * 10 * 4
    assert slabs(L, 4, 10, one - 1) == 0 and slabs(L, 4, 10, one) == 1 and slabs(L, 4, 10, 2 * one - 1) == 1 and slabs(L, 4, 10, 0) == 0
    assert slabs(L, 0, 10, -1) == -1 and 'conv2d_wgrad_stem_bf16_slabs' in L.last_error()
    assert slabs(L, 1, 0, -1) == -1


def test_wide_entries_refuse_other_channel_counts_before_any_device_call(L):
    """Fake device pointers, never dereferenced: the geometry is checked first."""
    c = L.lib.c
    X, Wp, Y, S = (ctypes.c_void_p(v) for v in (0x10000000, 0x20000000, 0x30000000, 0x40000000))
    want = 'geometry not supported (64 <= 7 * cin <= 95, win % 32 == 0)'
    for name in ENTRIES:
        fn = getattr(c, name)
        tail = (None, S, None) if '_fwd_' in name else (S, None)
        for cin in (1, 5, 9, 14, 64):
            assert fn(X, Wp, Y, 2, 96, 96, cin, *tail) == -1, (name, cin)
            assert name[len('simq_'):] + ': ' + want in L.last_error(), L.last_error()
        assert fn(X, Wp, Y, 2, 96, 80, 10, *tail) == -1 and want in L.last_error()          # win % 32
        assert fn(X, Wp, Y, 0, 96, 96, 10, *tail) == -1 and 'bad argument' in L.last_error()
        assert fn(None, Wp, Y, 2, 96, 96, 10, *tail) == -1 and 'bad argument' in L.last_error()
        if name.endswith('_x16'):
            assert fn(ctypes.c_void_p(0x10000001), Wp, Y, 2, 96, 96, 10, *tail) == -1 and 'd_x must be 2-byte aligned' in L.last_error()
    # the narrow entries keep refusing ten channels
    for name in ENTRIES:
        fn = getattr(c, name.replace('_wide', ''))
        tail = (None, S, None) if '_fwd_' in name else (S, None)
        assert fn(X, Wp, Y, 2, 96, 96, 10, *tail) == -1 and '7 * cin <= 63' in L.last_error(), name
