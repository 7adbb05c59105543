"""CPU: host-side logic of the product package -- config surface, plugin registry, state_dict contract,
C-ABI exports, LR schedule, synthetic batch contract, loud failure without the GPU."""
import ctypes
import json
import os
import re

import pytest
import torch

from _util import GOLDEN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_c_abi_exports_every_declared_symbol():
    """The product library loads and exports exactly what include/msmc_hip.h declares (no compute calls)."""
    import __graft_entry__ as g
    g.build()
    from msmctts_amd.hip import lib
    header = open(os.path.join(ROOT, 'include', 'msmc_hip.h')).read()
    declared = set(re.findall(r'\b(msmc_[a-z0-9_]+)\s*\(', header))
    assert declared == set(lib.exported_symbols())
    # the product ABI carries no process-global switch ("no hidden global state"): those live in the debug header
    assert not [n for n in declared if '_set_' in n], sorted(n for n in declared if '_set_' in n)
    debug = set(re.findall(r'\b(msmc_[a-z0-9_]+)\s*\(', open(os.path.join(ROOT, 'include', 'msmc_hip_debug.h')).read()))
    assert debug == set(lib.debug_symbols()) and not (debug & declared)
    handle = ctypes.CDLL(lib.DEFAULT_PATH)
    for name in declared | debug:
        assert hasattr(handle, name), name
    assert lib.load().msmc_backend() == b'gfx950'


def test_product_refuses_host_tensors_without_test_hook():
    from msmctts_amd.hip import lib
    saved = (lib._lib, lib._host_pointers_ok)
    try:
        lib._lib, lib._host_pointers_ok = lib.load(), False
        with pytest.raises(RuntimeError, match='GPU only'):
            lib.ptr(torch.zeros(4))
    finally:
        lib._lib, lib._host_pointers_ok = saved


def test_missing_library_fails_loudly(tmp_path):
    from msmctts_amd.hip import lib
    with pytest.raises(RuntimeError, match='not found'):
        lib.load(str(tmp_path / 'libmsmc_hip.so'))


def test_config_surface():
    from msmctts_amd.utils.config import Config, read_yaml
    p = os.path.join(GOLDEN, '_cfg.yaml')
    with open(p, 'w') as f:
        f.write('id: x\noptimizer:\n  _default:\n    learning_rate: 2e-4\n    name: None\ncudnn:\n  benchmark: True\n')
    try:
        c = Config(p)
        assert isinstance(c.optimizer._default.learning_rate, float) and c.optimizer._default.learning_rate == 2e-4
        assert c.optimizer._default.name is None
        assert c.cudnn.enabled is True and c.cudnn.benchmark is True            # merged over defaults
        assert c.distributed.dist_backend == 'nccl' and c.training_steps == 1000000
        assert c.to_dict()['optimizer']['_default']['learning_rate'] == 2e-4
        with pytest.raises(AttributeError):
            c.nope
    finally:
        os.remove(p)


def test_registry_and_state_dict_contract():
    import _parity
    _parity.check_state_dict_surface()
    from msmctts_amd.networks import find_modules
    with pytest.raises(RuntimeError):
        find_modules({'x': {'_name': 'NoSuchNetwork'}})
    from msmctts_amd.configs import csmsc_config
    nets = dict(find_modules({k: v for k, v in csmsc_config()['task'].items() if k[:1] != '_'}))
    assert type(nets['autoencoder']).__name__ == 'MSMCVQGAN'
    assert type(nets['discriminator']).__name__ == 'Discriminator'
    frozen = [n for n, p in nets['autoencoder'].named_parameters() if not p.requires_grad]
    assert frozen == ['encoder.encoders.0.position.weight', 'encoder.encoders.1.position.weight',
                      'frame_decoder.position.weight']


def test_multihead_buffers_are_views_of_packed_storage():
    from msmctts_amd.networks.vqgantts.modules import MultiHeadQuantize
    q = MultiHeadQuantize(32, 16, 4)
    e, c, a = q._packed()
    assert e.shape == (4, 8, 16) and c.shape == (4, 16)
    sd = {k: torch.full_like(v, float(i)) for i, (k, v) in enumerate(q.state_dict().items())}
    q.load_state_dict(sd)                                     # in-place copy keeps the packing
    e2, _, _ = q._packed()
    assert e2.data_ptr() == e.data_ptr()
    assert torch.equal(e2[1], sd['quantizers.1.embed'])
    q2 = q.double().float()                                  # _apply re-creates buffers -> repacked lazily
    e3, _, _ = q2._packed()
    assert torch.equal(e3[2], sd['quantizers.2.embed'])
    assert q2.quantizers[2].embed.data_ptr() == e3[2].data_ptr()


def test_lr_schedule_matches_reference():
    from msmctts_amd.trainers.lr_schedulers import build_lr_scheduler
    with open(os.path.join(GOLDEN, 'schedule.json')) as f:
        s = json.load(f)
    sch = build_lr_scheduler(dict(_name='ExponentialDecayLRScheduler', warmup_steps=200000, decay_scale=200000,
                                  decay_learning_rate=0.5, final_learning_rate=1e-5))
    for step, lr in zip(s['lr_steps'], s['lr_values']):
        assert abs(max(1e-5, sch.get_scale(step) * 2e-4) - lr) < 1e-12


def test_synthetic_batch_contract():
    from msmctts_amd.synthetic import make_batch
    b = make_batch(8, 40, 80, 300, seed=1, rank=0)
    ln = b['mel_length']
    assert b['mel'].shape == (8, 40, 80) and b['wav'].shape == (8, 12000, 1) and ln.dtype == torch.int64
    assert int(ln.max()) == 40 and bool((ln[:-1] >= ln[1:]).all()) and int(ln.min()) >= 20
    assert torch.equal(b['wav_length'], ln * 300)
    for i, l in enumerate(ln.tolist()):
        assert bool((b['mel'][i, l:] == -4).all()) and bool((b['wav'][i, l * 300:] == 0).all())
    b2 = make_batch(8, 40, 80, 300, seed=1, rank=1)
    assert not torch.equal(b['mel'], b2['mel'])


def test_every_decision_of_the_shipped_table_names_a_kernel_the_library_still_has():
    """hip/tuned_gfx950.json against the candidate lists of hip/conv.py: a retired kernel configuration (round 6 refused and
    de-instantiated gather3 22 / 23 / 30, gather5 43 and four weight-gradient candidates) must not survive in a decision --
    the launch it selects would fail at run time on the one shape that kept it"""
    from msmctts_amd.hip import conv
    gather = {v for v, _ in conv._GATHER_CANDIDATES}
    wgrad = set(conv._WGRAD_CANDIDATES)
    uniform = {v for v, _ in conv._UNIFORM_CANDIDATES} if isinstance(conv._UNIFORM_CANDIDATES[0], tuple) else set(conv._UNIFORM_CANDIDATES)
    split = {v for v, _ in conv._SPLIT_CANDIDATES}
    assert len(conv.TUNED) > 1000
    for key, dec in conv.TUNED.items():
        kind = key[0]
        if kind == 'gather':
            assert dec[0] in gather, (key, dec[:2])
        elif kind == 'wgrad':
            assert (dec[0], dec[1]) in wgrad, (key, dec[:2])
        elif kind == 'gather-split':
            assert dec[0] in split, (key, dec[:2])
        elif kind == 'gather-group':
            assert dec[0] in (0, 1, 3) and (dec[0] != 3 or dec[1] in uniform), (key, dec[:2])
        elif kind == 'wgrad-group':
            assert dec[0] in (0, 1, 2), (key, dec[:2])
        else:
            raise AssertionError('unknown kind of decision: %r' % (kind,))


def test_tuner_borrows_the_nearest_tuned_shape_of_the_same_class():
    """variable-length batches: a new padded length does not trigger timing launches when a shape of the same
    channel / tap / stride class is already tuned; the nearest pixel count wins; another class does not match"""
    from msmctts_amd.hip import conv as K
    keep = dict(K.TUNED)
    try:
        K.TUNED.clear()
        taps = ((0, 0, 0), (0, 1, 2))
        sig = lambda T, cin=256: ('gather', 1, 16, 1, T, cin, 1, T, 1024, 1, T, 1, 1, 1, 1, 3, taps[0], taps[1], 0, False,
                                  False, False)
        K.TUNED[sig(400)] = (19, 0, {})
        K.TUNED[sig(100)] = (9, 0, {})
        assert K._nearest_tuned(sig(380))[0] == 19
        assert K._nearest_tuned(sig(120))[0] == 9
        assert K._nearest_tuned(sig(380, cin=128)) is None
        cache = {i: i for i in range(5000)}
        K._bounded(cache, 4096)
        assert not cache
    finally:
        K.TUNED.clear()
        K.TUNED.update(keep)
        K._CLASS_INDEXED[0] = -1


def test_bench_line_is_one_short_parseable_json_line(tmp_path):
    """The driver parses ONE JSON line from bench.py's stdout; round 2's line (36 KB with the per-kernel table inline)
    came back unparsed.  emit_line moves the table to a side file and keeps the line under 8 KB whatever the table's
    size, without touching the contract keys, `roofline` or `cpu_baseline`."""
    import bench
    full = json.load(open(os.path.join(ROOT, 'profiles', 'r02_bench.json')))
    assert len(json.dumps(full)) > 30000 and 'kernels' in full            # the line that did not parse
    side = str(tmp_path / 'sub' / 'kernels.json')
    line = bench.emit_line(full, side)
    assert '\n' not in line and len(line) < 8192
    got = json.loads(line)
    for key in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
                'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert got[key] == full[key], key
    assert 'kernels' not in got and got['kernels_file']
    assert json.load(open(side))['kernels'] == full['kernels']
    # a pathologically long optional block is dropped before the line may exceed the limit
    fat = dict(full, vq_microbench=[{'note': 'x' * 9000}])
    slim = json.loads(bench.emit_line(fat, None))
    assert 'vq_microbench' not in slim and slim['roofline'] == {k: v for k, v in full['roofline'].items() if k != 'note'}
    assert slim['cpu_baseline']['value'] == full['cpu_baseline']['value']


def test_bench_dump_outputs_writes_what_the_step_returned(tmp_path, monkeypatch):
    """``bench.py --dump-outputs DIR``: every tensor / number of the structure ``train_step`` returned becomes
    ``DIR/<dotted name>.npy`` with its values, float32 (float64 for 64-bit values); above the size limit each array larger
    than its share is cut to the same seeded sample on every call, so two builds can be compared file by file."""
    import numpy as np
    import bench
    log = {'loss': {'mel': torch.tensor(1.25, dtype=torch.bfloat16), 'vq': torch.arange(6, dtype=torch.float64).reshape(2, 3), 'n': 3},
           'big': torch.arange(4096, dtype=torch.float32)}
    bench.dump_outputs(str(tmp_path / 'a'), log)
    got = {f[:-4]: np.load(str(tmp_path / 'a' / f)) for f in os.listdir(str(tmp_path / 'a'))}
    assert set(got) == {'loss.mel', 'loss.vq', 'loss.n', 'big'}
    assert got['loss.mel'].dtype == np.float32 and got['loss.mel'] == 1.25
    assert got['loss.vq'].dtype == np.float64 and np.array_equal(got['loss.vq'], np.arange(6.0).reshape(2, 3))
    assert got['loss.n'] == 3.0 and np.array_equal(got['big'], np.arange(4096, dtype=np.float32))
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 4096)
    bench.dump_outputs(str(tmp_path / 'b'), log)
    bench.dump_outputs(str(tmp_path / 'c'), log)
    small = {f[:-4]: np.load(str(tmp_path / 'b' / f)) for f in os.listdir(str(tmp_path / 'b'))}
    assert sum(a.nbytes for a in small.values()) <= 4096 and small['big'].size == 256 and len(set(small['big'])) == 256
    assert np.array_equal(small['loss.vq'], got['loss.vq']) and np.array_equal(small['big'], np.load(str(tmp_path / 'c' / 'big.npy')))


def _header_struct_fields(name):
    """[(field, kind)] of ``typedef struct <name> {...}`` in include/msmc_hip.h; kind: 'p' pointer, 'i' int, 'f' float,
    'l' long, ('i', n) int array"""
    header = open(os.path.join(ROOT, 'include', 'msmc_hip.h')).read()
    body = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    out = []
    for stmt in body.split(';'):
        stmt = ' '.join(stmt.split())
        if not stmt:
            continue
        m = re.match(r'(const )?(void|float|int|long)( ?\*)? ?(.*)', stmt)
        assert m, stmt
        base, ptr = m.group(2), bool(m.group(3))
        for decl in m.group(4).split(','):
            decl = decl.strip()
            arr = re.match(r'(\w+)\[(\w+)\]', decl)
            if ptr or decl.startswith('*'):
                out.append((decl.lstrip('* '), 'p'))
            elif arr:
                n = {'MSMC_CONV_MAX_TAPS': 16, 'MSMC_MAX_TENSORS': 64}.get(arr.group(2)) or int(arr.group(2))
                out.append((arr.group(1), (base[0], n)))
            else:
                out.append((decl, base[0]))
    return out


def test_conv_descriptor_is_the_same_in_header_binding_and_integration_doc():
    """include/msmc_hip.h `msmc_conv_desc`, the ctypes binding (hip/lib.py ConvDesc) and the struct a maintainer would
    copy from INTEGRATION.md route B agree field for field, in order (round 2: the doc block was three ints short)."""
    from msmctts_amd.hip import lib
    want = _header_struct_fields('msmc_conv_desc')
    kinds = {ctypes.c_void_p: 'p', ctypes.c_int: 'i', ctypes.c_float: 'f', ctypes.c_long: 'l'}

    def kind(ct):
        return kinds[ct] if ct in kinds else (kinds[ct._type_], ct._length_)
    assert [(n, kind(ct)) for n, ct in lib.ConvDesc._fields_] == want
    doc = open(os.path.join(ROOT, 'INTEGRATION.md')).read()
    block = re.search(r'class msmc_conv_desc\(ctypes\.Structure\):.*?_fields_ = \[(.*?)\]\n', doc, re.S).group(1)
    got = []
    for n, ct, arr in re.findall(r"\('(\w+)', ctypes\.c_(\w+)( \* \d+)?\)", block):
        k = {'void_p': 'p', 'int': 'i', 'float': 'f', 'long': 'l'}[ct]
        got.append((n, (k, int(arr.strip(' *'))) if arr else k))
    assert got == want
    assert ctypes.sizeof(lib.ConvDesc) == 360         # 7 pointers, 68 + 3 ints, 4 floats, padded to 8 bytes
    # the other by-value structs of the ABI, binding against header
    for cname, cls in (('msmc_opt_tensor', lib.OptTensor), ('msmc_wn_item', lib.WnItem)):
        assert [n for n, _ in cls._fields_] == [n for n, _ in _header_struct_fields(cname)], cname


@pytest.mark.parametrize('case', ['csmsc', 'decay', 'default'])
def test_radam_matches_the_reference_optimizer(case):
    """``optimizer._name: RAdam`` (reference trainers/optimizers/__init__.py:8-21, radam.py:8-85) against parameters and
    moments the reference's own class produced (tests/golden/make_golden_radam.py): eight steps through both branches of
    the variance rectification, with and without weight decay, and with the class defaults."""
    import numpy as np
    from msmctts_amd.trainers.optimizers.radam import RAdam
    kw = {'csmsc': dict(lr=2e-4, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.0),
          'decay': dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01), 'default': {}}[case]
    z = np.load(os.path.join(GOLDEN, 'radam_cases.npz'))
    n = len([k for k in z.files if k.startswith(case + '/p0/')])
    params = [torch.nn.Parameter(torch.from_numpy(z['%s/p0/%d' % (case, i)].copy())) for i in range(n)]
    opt = RAdam(params, **kw)
    for t in range(8):
        for i, p in enumerate(params):
            p.grad = torch.from_numpy(z['%s/g%d/%d' % (case, t, i)].copy())
        opt.step()
        for i, p in enumerate(params):
            want = z['%s/p%d/%d' % (case, t + 1, i)]
            assert np.allclose(p.detach().numpy(), want, rtol=0, atol=1e-6), (case, t, i, np.abs(p.detach().numpy() - want).max())
    for i, p in enumerate(params):
        st = opt.state[p]
        assert int(st['step']) == int(z['%s/step/%d' % (case, i)])
        assert np.allclose(st['exp_avg'].numpy(), z['%s/exp_avg/%d' % (case, i)], rtol=0, atol=1e-6)
        assert np.allclose(st['exp_avg_sq'].numpy(), z['%s/exp_avg_sq/%d' % (case, i)], rtol=0, atol=1e-6)


def test_radam_is_selectable_from_the_optimizer_section():
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.trainers.optimizers.radam import RAdam
    from msmctts_amd.utils.config import Config
    model = torch.nn.Module()
    model.add_module('autoencoder', torch.nn.Linear(3, 2))
    cfg = Config({'optimizer': {'_default': dict(_name='RAdam', learning_rate=1e-3, betas=[0.5, 0.9], eps=1e-8, weight_decay=0.0)}})
    bundle = build_optimizer(model, cfg.optimizer)
    assert isinstance(bundle.optimizers['autoencoder'], RAdam)
    model.autoencoder.weight.grad = torch.ones(2, 3)
    model.autoencoder.bias.grad = torch.ones(2)
    before = model.autoencoder.weight.detach().clone()
    bundle.step(['autoencoder'])
    assert not torch.equal(before, model.autoencoder.weight)


REF_CONFIGS = '/root/reference/examples/csmsc/configs'


@pytest.mark.skipif(not os.path.isdir(REF_CONFIGS), reason='build-container test: needs the reference tree (never on the GPU box)')
@pytest.mark.parametrize('name,mode,children', [('msmc_vq_gan.yaml', 'train', {'autoencoder': 0, 'discriminator': 0}),
                                                ('msmc_vq_gan_am.yaml', 'train', {'predictor': 0})])
def test_the_reference_yaml_files_load_unchanged(name, mode, children):
    """The reference's own configuration files (examples/csmsc/configs/*.yaml) through Config -> build_task ->
    build_trainer -> build_optimizer of this package: the plug-in names resolve, the constructors take the YAML's
    keywords, and the checkpoint surface is the reference's (636 keys for the autoencoder + discriminator task,
    tests/golden/schedule.json)."""
    from msmctts_amd.tasks import build_task
    from msmctts_amd.trainers import build_trainer
    from msmctts_amd.trainers.optimizers import build_optimizer
    from msmctts_amd.utils.config import Config
    cfg = Config(os.path.join(REF_CONFIGS, name))
    task = build_task(cfg, mode=mode)
    assert set(n for n, _ in task.named_children()) >= set(children)
    trainer = build_trainer(cfg, task, num_gpus=0, rank=0)
    trainer.optimizer = build_optimizer(task, cfg.optimizer)
    assert type(trainer).__name__ == cfg.trainer._name
    sd = task.state_dict()
    if name == 'msmc_vq_gan.yaml':
        want = json.load(open(os.path.join(GOLDEN, 'schedule.json')))['csmsc_state_dict']
        assert want == [[k, list(v.shape)] for k, v in sd.items()]


def test_interpreter_runtime_declares_the_same_primitives_as_the_gfx950_runtime():
    """tests/emu/msmc_rt.hpp is a hand-kept CPU twin of csrc/gfx950/msmc_rt.hpp (the kernels include whichever the build
    puts on the include path): every device primitive, macro and vector type one of them declares must exist in the other,
    so that a primitive added for a new kernel cannot silently be missing -- or mean something else by accident of a stale
    copy -- on the interpreter.  (Internals of the gfx950 file that kernels never call are listed.)"""
    def names(path):
        s = open(path).read()
        fn = set(re.findall(r'MSMC_DEV(?:_INLINE)?\s+[\w:<>\*& ]+?\s+(\w+)\s*\(', s))
        mac = set(re.findall(r'#define\s+(MSMC_\w+)', s))
        typ = set(re.findall(r'typedef\s+[^;]*?\s(\w+)\s+__attribute__', s))
        return s, fn, mac, typ
    gs, gfn, gmac, gtyp = names(os.path.join(ROOT, 'msmc-tts_amd', 'csrc', 'gfx950', 'msmc_rt.hpp'))
    es, efn, emac, etyp = names(os.path.join(ROOT, 'tests', 'emu', 'msmc_rt.hpp'))
    internal = {'wave_dpp_t', 'wave_xor16_u', 'wave_xor32_u'}           # building blocks of wave_sum / wave_xor16 / wave_xor32
    local_types = {'bf16x2_', 'f32x2_', 's16x4_'}                       # typedefs inside function bodies
    missing = [n for n in sorted(gfn - internal) if not re.search(r'\b%s\s*\(' % n, es)]
    assert not missing, 'primitives of the gfx950 runtime the interpreter does not provide: %s' % missing
    extra = [n for n in sorted(efn) if not re.search(r'\b%s\s*\(' % n, gs)]
    assert not extra, 'interpreter-only primitives (a kernel using one would not build for the GPU): %s' % extra
    assert gmac == emac, (sorted(gmac - emac), sorted(emac - gmac))
    assert gtyp - local_types == etyp - local_types, (sorted(gtyp - etyp), sorted(etyp - gtyp))
    # every primitive the kernel sources call is one both files know
    csrc = os.path.join(ROOT, 'msmc-tts_amd', 'csrc')
    used = set()
    for f in os.listdir(csrc):
        if f.endswith(('.hip', '.inc')):
            text = open(os.path.join(csrc, f)).read()
            used |= {n for n in gfn if re.search(r'\b%s\s*(<[^;(]*>)?\s*\(' % n, text)}
    assert len(used) >= 25, sorted(used)


def test_bench_watchdog_guard_turns_a_stalled_secondary_measurement_into_a_line_and_exit_0(tmp_path):
    """bench.py at N > 1 times the untried exchange modes AFTER the headline, under ``Watchdog.guard``: a stall there must
    print what rank 0 has and end the process with exit code 0 (a stall before it: exit 5, nothing printed)."""
    import subprocess
    import sys
    code = (
        "import sys, time; sys.path.insert(0, %r); import bench\n"
        "wd = bench.Watchdog(1.0, 0)\n"
        "if sys.argv[1] == 'guarded':\n"
        "    wd.guard(lambda what: print('LINE after ' + what), 1.0)\n"
        "wd.beat('the untried mode')\n"
        "time.sleep(30)\n" % ROOT)
    r = subprocess.run([sys.executable, '-c', code, 'guarded'], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and 'LINE after the untried mode' in r.stdout, (r.returncode, r.stdout, r.stderr[-300:])
    r = subprocess.run([sys.executable, '-c', code, 'plain'], capture_output=True, text=True, timeout=60)
    assert r.returncode == 5 and 'LINE' not in r.stdout, (r.returncode, r.stdout, r.stderr[-300:])
