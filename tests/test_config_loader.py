"""load_config: the reference's config format (JSON with // comments, layered through "configBase").  The reference's own
bench and CC11xx configs, as load_config read them (fixture tests/golden/ref_configs.json, recorded by
tests/golden/make_golden_configs.py), are compared with the dictionaries our builders produce, on every key the
demodulator reads."""
import json
import os

import pytest

from pycusdr_amd import config as cfg

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ref_configs.json')


@pytest.fixture(scope='module')
def ref_configs():
    with open(GOLDEN) as f:
        return json.load(f)


def test_comments_layers_and_overrides(tmp_path):
    (tmp_path / 'base.json').write_text('''// base
{
  "Main": {"workerId": "base", "keep": 1}, /* block
  comment */
  "GPU": {"UHF": {"blockSize": 16, "CUDA": {"device": 0, "streams": 3}}},
  "Interfaces": {"in": "tcp://*:5512" // a URL is not a comment
  }
}''')
    sub = tmp_path / 'sub'
    sub.mkdir()
    (sub / 'mid.json').write_text('{"configBase": "../base.json", "GPU": {"UHF": {"blockSize": 15}}, "Main": {"workerId": "mid"}}')
    (sub / 'top.json').write_text('{"configBase": "mid.json", // chain\n "GPU": {"UHF": {"CUDA": {"device": 3}}}, "text": "a \\"q\\" // not a comment"}')
    c = cfg.load_config(sub / 'top.json')
    assert c['Main'] == {'workerId': 'mid', 'keep': 1}
    assert c['GPU']['UHF'] == {'blockSize': 15, 'CUDA': {'device': 3, 'streams': 3}}
    assert c['Interfaces']['in'] == 'tcp://*:5512' and c['text'] == 'a "q" // not a comment'
    assert 'configBase' not in c
    (sub / 'loop.json').write_text('{"configBase": "loop.json"}')
    with pytest.raises(ValueError):
        cfg.load_config(sub / 'loop.json')


@pytest.mark.parametrize('name', ['bench_GMSK', 'bench_FSK', 'bench_GFSK', 'bench_BPSK'])
def test_reference_bench_configs_equal_our_builder(ref_configs, name):
    ref = ref_configs[name]
    ours = cfg.bench_config(name, blockSize=ref['GPU']['UHF']['blockSize'])
    assert ref['Main']['protocols']['UHF'] == name == ours['Main']['protocols']['UHF']
    for k in ('PacketLen', 'RandSeed'):
        assert ref['Main'][k] == ours['Main'][k]
    assert ref['Radios']['rangeRateMax'] == ours['Radios']['rangeRateMax']
    r, o = ref['Radios']['Rx']['UHF-H'], ours['Radios']['Rx']['UHF-H']
    for k in ('CUDA_settings', 'frequency_Hz', 'frequencyOffset_Hz', 'baud', 'samplesPerSym', 'doppCarrierSteps', 'Protocol', 'radioBackend'):
        assert r[k] == o[k], k
    for gpu_set in ('UHF', 'STX'):
        for k, v in ours['GPU'][gpu_set].items():
            assert ref['GPU'][gpu_set][k] == v, (gpu_set, k)


def test_reference_cc11xx_config_equals_our_builder(ref_configs):
    ref = ref_configs['CC11xx']
    ours = cfg.cc11xx_config(blockSize=ref['GPU']['UHF']['blockSize'])
    rx_name = next(iter(ours['Radios']['Rx']))
    r = ref['Radios']['Rx'][rx_name] if rx_name in ref['Radios']['Rx'] else next(iter(ref['Radios']['Rx'].values()))
    o = ours['Radios']['Rx'][rx_name]
    for k in ('frequency_Hz', 'frequencyOffset_Hz', 'baud', 'samplesPerSym', 'radioBackend'):
        assert r[k] == o[k], k
    assert ref['Radios']['rangeRateMax'] == ours['Radios']['rangeRateMax']
    for k in ('rx_preamble', 'rx_sync_seq'):
        assert ref['Radios']['Protocol'][k] == ours['Radios']['Protocol'][k], k
