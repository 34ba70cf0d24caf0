"""The entropy choice through the loader and the driver, host half only (no GPU): DeviceLoader(device=None, entropy='device') prepares
the same samples as the host loader, its worker leaves streams where the host path leaves coefficients, and file_datasets reads
training.jpeg_entropy / GPV_JPEG_ENTROPY."""
import numpy as np
import pytest

from tests import coco_tree as CT

PLAN = {'cap': {'train': [2], 'val': [2, 3]}, 'det': {'train': [4], 'val': [4]}, 'cls': {'train': [1]}, 'vqa': {'train': [3]},
        'refcocop': {'train': [6]}}
KINDS = ('cap', 'det', 'cls', 'vqa', 'refcocop')


def test_host_half_of_the_device_route_matches_the_host_loader(tmp_path):
    import gpv1_amd.hip as hip
    from gpv1_amd import jpeg_entropy as E
    from gpv1_amd.datasets import CocoMultitaskDataset, DeviceLoader
    tc = CT.make_tree(tmp_path, PLAN, image_size=(64, 96))
    groups = [[3, 0], [2, 4], [1, 0]]
    got = {}
    for entropy in ('host', 'device'):
        ds = CocoMultitaskDataset(CT.learning_datasets(KINDS), tc, 'train', seed=5)
        loader = DeviceLoader(ds, 2, device=None, threads=2, prefetch=1, entropy=entropy)
        assert loader.dec.entropy == entropy
        got[entropy] = list(loader.host_batches(groups, epoch=2))
        loader.close()
    routed = 0
    for a, b in zip(got['host'], got['device']):
        assert (a.indices, a.paths, a.params, a.crops, a.queries) == (b.indices, b.paths, b.params, b.crops, b.queries)
        assert a.parsed.huff is None and b.parsed.huff is not None
        assert [bytes(x) for x in a.parsed.infos] == [bytes(x) for x in b.parsed.infos]
        on_dev = {i: (desc, at) for i, desc, at in b.parsed.huff}
        routed += len(on_dev)
        blob = b.parsed.coefs.numpy()
        for i, path in enumerate(b.paths):
            data = open(path, 'rb').read()
            if i in on_dev:
                desc, at = on_dev[i]
                prep = E.prepare_host(data)
                assert prep['route'] == 'device' and at % 16 == 0 and desc.nbits == prep['nbits']
                assert blob.view(np.uint8)[at:at + desc.stream_cap].tobytes() == prep['stream'].tobytes()
            else:                                                         # routed to the host: the coefficients, as before
                n = int(b.parsed.infos[i].coef_count)
                ref = np.zeros(n, np.int16)
                hip.jpeg_parse(data, ref)
                assert np.array_equal(blob[b.parsed.starts[i]:b.parsed.starts[i] + n], ref)
    assert routed >= 1


def test_driver_reads_the_config_key_and_the_environment(tmp_path, monkeypatch):
    from gpv1_amd import train_distr as td
    from gpv1_amd.misc import AttrDict
    tc = CT.make_tree(tmp_path, PLAN, image_size=(64, 96))

    def cfg(**training):
        return AttrDict({'training': AttrDict(dict({'num_workers': 2, 'prefetch': 0, 'batch_size': 2}, **training)), 'seed': 0,
                         'learning_datasets': CT.learning_datasets(KINDS), 'task_configs': tc})
    monkeypatch.delenv('GPV_JPEG_ENTROPY', raising=False)
    ds, _ = td.file_datasets(cfg(), 2, None, evals=False)
    assert ds.loader.dec.entropy == 'host'
    ds, _ = td.file_datasets(cfg(jpeg_entropy='device'), 2, None, evals=False)
    assert ds.loader.dec.entropy == 'device'
    monkeypatch.setenv('GPV_JPEG_ENTROPY', 'device')
    ds, _ = td.file_datasets(cfg(), 2, None, evals=False)
    assert ds.loader.dec.entropy == 'device'
    monkeypatch.setenv('GPV_JPEG_ENTROPY', 'nowhere')
    with pytest.raises(ValueError, match='entropy'):
        td.file_datasets(cfg(), 2, None, evals=False)
    import gpv1_amd.default_config as dc
    assert 'jpeg_entropy' not in open(dc.__file__).read()
