"""CPU: what the one-call intention supervision step and the typed intention kernels fix before they need a
device -- the new names in the header, the library and the ctypes table, the size of simq_intention_args on both sides, and the
refusals that are decided before anything is launched."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ('simq_intention_split', 'simq_bce_with_logits_state', 'simq_bce_state_scratch_bytes', 'simq_sigmoid_concat_x',
       'simq_train_intention_step')
OLD = ('simq_split_last_channel', 'simq_bce_with_logits', 'simq_sigmoid_concat')


@pytest.fixture(scope='module')
def L():
    import __graft_entry__ as ge
    ge.build()
    from simq import _lib
    return _lib


def header_text():
    return re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'simq.h')).read(), flags=re.S)


def test_new_names_are_declared_exported_and_bound(L):
    header = header_text()
    raw = ctypes.CDLL(L.LIB_PATH)
    dynamic = subprocess.run(['nm', '-D', '--defined-only', L.LIB_PATH], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in dynamic.splitlines() if line.strip()}
    for name in NEW + OLD:
        proto = re.search(r'\b%s\s*\(([^;]*)\)\s*;' % name, header)
        assert proto, '%s is not declared in include/simq.h' % name
        assert hasattr(raw, name) and name in exported, 'libsimq.so does not export %s' % name
        nargs = 0 if proto.group(1).strip() == 'void' else proto.group(1).count(',') + 1
        assert name in L.EXPORTS and len(L._SIGS[name][1]) == nargs, name
    assert L.lib.version == 500                                                   # new entries, no change to an existing one
    assert L._c.simq_bce_state_scratch_bytes() >= 8 and L._c.simq_bce_state_scratch_bytes() % 8 == 0


def c_sizeof(struct_name, tmp_path):
    """sizeof(struct) as the host C compiler lays the header's struct out."""
    src = tmp_path / 'size.c'
    src.write_text('#include <stdio.h>\n#include "simq.h"\nint main(void) { printf("%%zu\\n", sizeof(%s)); return 0; }\n' % struct_name)
    exe = tmp_path / 'size'
    cc = next(c for c in ('cc', 'gcc', 'clang', '/opt/rocm/llvm/bin/clang') if subprocess.run(['sh', '-c', 'command -v %s' % c], stdout=subprocess.PIPE).returncode == 0)
    subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], check=True)
    return int(subprocess.run([str(exe)], stdout=subprocess.PIPE, text=True, check=True).stdout)


def test_intention_args_has_the_headers_size(L, tmp_path):
    body = re.search(r'typedef struct simq_intention_args \{(.*?)\} simq_intention_args;', header_text(), flags=re.S).group(1)
    names = [n for decl in body.split(';') for n in re.findall(r'[*\s,](\w+)\s*(?=,|$)', decl.strip())]
    assert names == [n for n, _ in L.IntentionArgs._fields_]                      # the same fields in the same order
    assert 'comm' not in names                                                    # data-parallel intention steps keep the separate calls
    assert ctypes.sizeof(L.IntentionArgs) == c_sizeof('simq_intention_args', tmp_path)
    assert ctypes.sizeof(L.TrainArgs) == c_sizeof('simq_train_args', tmp_path)    # (the neighbour did not move)
    # ... and the library was compiled from that header: a struct that names its true size gets past the size check
    a = L.IntentionArgs()
    a.plan = L.Plan(4, 1).handle
    a.struct_bytes = ctypes.sizeof(L.IntentionArgs)
    assert L._c.simq_train_intention_step(ctypes.byref(a)) != 0 and 'NULL buffer' in L.last_error()


def test_refusals_that_need_no_device(L):
    c = L._c
    assert c.simq_train_intention_step(None) != 0 and 'NULL' in L.last_error()
    plan = L.Plan(4, 1)
    a = L.IntentionArgs()
    a.plan = plan.handle
    a.batch, a.channels = 2, 5
    for wrong in (0, ctypes.sizeof(L.IntentionArgs) - 8, ctypes.sizeof(L.IntentionArgs) + 8, ctypes.sizeof(L.TrainArgs)):
        a.struct_bytes = wrong
        assert c.simq_train_intention_step(ctypes.byref(a)) != 0 and 'struct_bytes' in L.last_error()
    a.struct_bytes = ctypes.sizeof(L.IntentionArgs)
    assert c.simq_train_intention_step(ctypes.byref(a)) != 0 and 'NULL buffer' in L.last_error()
    # every buffer named (addresses that are never dereferenced: each refusal below comes before the first launch)
    fake = 1 << 20
    for k, (n, t) in enumerate(L.IntentionArgs._fields_):
        if t is ctypes.c_void_p and n not in ('plan', 'target', 'total_norm', 'loss_host', 'stream', 'side_stream'):
            setattr(a, n, fake * (k + 1))

    def refused(what, **fields):
        saved = {n: getattr(a, n) for n in fields}
        for n, v in fields.items():
            setattr(a, n, v)
        rc = c.simq_train_intention_step(ctypes.byref(a))
        msg = L.last_error()
        for n, v in saved.items():
            setattr(a, n, v)
        assert rc != 0 and what in msg, (fields, rc, msg)

    refused('channels', channels=1)                                               # C = 1: no head
    refused('channels', channels=4)                                               # the plan reads 4 channels, states of 4 leave 3
    refused('channels', channels=6)
    refused('state_bf16', state_bf16=2)
    refused('batch', batch=0)
    refused('batch', batch=4097)
    for n in ('params', 'wcache', 'bnbuf', 'grads', 'momentum_buf', 'ws_train', 'state', 'head', 'logits', 'dlogits', 'loss_sum', 'bce_scratch',
              'opt_scratch'):
        refused('NULL buffer', **{n: None})
    two_out = L.IntentionArgs.from_buffer_copy(a)
    two_out.plan = L.Plan(4, 2).handle
    assert c.simq_train_intention_step(ctypes.byref(two_out)) != 0 and 'one output channel' in L.last_error()

    # the three kernels' own entries
    p = ctypes.c_void_p
    assert c.simq_intention_split(p(256), 0, p(1 << 20), 0, None, 10, 1, None) != 0 and 'channels' in L.last_error()           # C = 1
    assert c.simq_intention_split(None, 0, p(1 << 20), 0, None, 10, 5, None) != 0 and 'NULL' in L.last_error()
    assert c.simq_intention_split(p(256), 0, None, 0, None, 10, 5, None) != 0 and 'NULL' in L.last_error()
    assert c.simq_intention_split(p(256), 2, p(1 << 20), 0, None, 10, 5, None) != 0 and 'element type' in L.last_error()
    assert c.simq_intention_split(p(256), 0, p(1 << 20), 0, None, 0, 5, None) != 0 and 'pixels' in L.last_error()
    assert c.simq_intention_split(p(258), 0, p(1 << 20), 0, None, 10, 5, None) != 0 and 'aligned' in L.last_error()             # fp32 at 2 mod 4
    assert c.simq_intention_split(p(257), 1, p(1 << 20), 1, None, 10, 5, None) != 0 and 'aligned' in L.last_error()             # bf16 at an odd address
    assert c.simq_intention_split(p(256), 0, p(256 + 40), 0, None, 10, 5, None) != 0 and 'overlaps' in L.last_error()           # head inside the state
    assert c.simq_intention_split(p(256), 0, p(1 << 20), 0, p(256 + 16), 10, 5, None) != 0 and 'overlaps' in L.last_error()     # last inside the state
    assert c.simq_bce_with_logits_state(None, p(256), 0, 10, 5, None, p(1 << 20), p(1 << 21), None) != 0 and 'NULL' in L.last_error()
    assert c.simq_bce_with_logits_state(p(1 << 12), p(256), 0, 10, 5, None, None, p(1 << 21), None) != 0 and 'NULL' in L.last_error()
    assert c.simq_bce_with_logits_state(p(1 << 12), p(256), 0, 10, 5, None, p(1 << 20), None, None) != 0 and 'NULL' in L.last_error()     # no scratch
    assert c.simq_bce_with_logits_state(p(1 << 12), p(256), 0, 10, 0, None, p(1 << 20), p(1 << 21), None) != 0 and 'channels' in L.last_error()
    assert c.simq_bce_with_logits_state(p(1 << 12), p(256), 0, 10, 5, None, p((1 << 20) + 4), p(1 << 21), None) != 0 and 'aligned' in L.last_error()
    assert c.simq_bce_with_logits_state(p(1 << 12), p(256), 0, 10, 5, None, p(1 << 21), p(1 << 21), None) != 0 and 'overlaps' in L.last_error()
    assert c.simq_sigmoid_concat_x(None, 0, p(1 << 12), p(1 << 20), 0, None, 10, 4, None) != 0 and 'NULL' in L.last_error()
    assert c.simq_sigmoid_concat_x(p(256), 0, p(1 << 12), p(1 << 20), 3, None, 10, 4, None) != 0 and 'element type' in L.last_error()
    assert c.simq_sigmoid_concat_x(p(256), 0, p(1 << 12), p(1 << 20), 0, None, 10, 0, None) != 0 and 'channels' in L.last_error()
    assert c.simq_sigmoid_concat_x(p(256), 0, p(1 << 12), p(256 + 64), 0, None, 10, 4, None) != 0 and 'overlaps' in L.last_error()


def test_comm_with_the_fused_step_is_refused_before_anything_else():
    """fused=True is single-process: a communicator or a process group is refused before the net, the batch or a device is looked at."""
    from simq import learner
    from simq._lib import SimqError
    with pytest.raises(SimqError, match='single-process'):
        learner.train_intention_step(object(), None, 0.01, 0.9, 1e-4, comm=object(), fused=True)
    with pytest.raises(SimqError, match='single-process'):
        learner.train_intention_step(object(), None, 0.01, 0.9, 1e-4, process_group=object(), fused=True)

    class Net:                                                                    # fused=None reads the net's attribute
        fused_step = True
    with pytest.raises(SimqError, match='single-process'):
        learner.train_intention_step(Net(), None, 0.01, 0.9, 1e-4, comm=object())
    with pytest.raises(SimqError, match='needs a simq.FCN'):                      # without it: today's first check
        learner.train_intention_step(object(), None, 0.01, 0.9, 1e-4, comm=object())
