"""Handle lifetime on the device: create -> one forward -> close(), three times per model.  A handle owns its weight image
(and, for the x3-core models, a second allocation of the same order with the weight planes); a create/destroy pair that left
either behind would lower the free device memory by at least two weight images over the two later cycles — the test allows
less than one.  Normal create / destroy only."""
import gc

import pytest
import torch

pytestmark = pytest.mark.gpu
dev = torch.device("cuda:0")


def _mf2():
    from targetdiarization_amd.separator import MossFormer2Separator
    from targetdiarization_amd.weights import pack_blob, recipe_state_dict
    sd = recipe_state_dict(seed=1, num_blocks=2)
    return len(pack_blob(sd)), lambda: MossFormer2Separator(sd, device=dev, num_blocks=2), lambda m: m(torch.zeros(1, 16, device=dev))


def _pfenc():
    from targetdiarization_amd.paraformer import ParaformerEncoder
    from targetdiarization_amd.weights import pack_blob, recipe_paraformer_state_dict
    sd = recipe_paraformer_state_dict(0, 2)
    return len(pack_blob(sd)), lambda: ParaformerEncoder(sd, dev, num_blocks=2), lambda m: m.encode(torch.zeros(1, 1, 560, device=dev))


def _eres2net():
    from targetdiarization_amd.speaker import ERes2NetV2
    from targetdiarization_amd.weights import pack_blob, recipe_eres2netv2_state_dict
    sd = recipe_eres2netv2_state_dict(0)
    return len(pack_blob(sd)), lambda: ERes2NetV2(sd, dev), lambda m: m.embed_features(torch.zeros(1, 9, 80, device=dev))


def _fsmn_vad():
    from targetdiarization_amd.vad import FsmnVad
    from targetdiarization_amd.weights import pack_fsmn_vad_blob, recipe_fsmn_vad_state_dict
    sd = recipe_fsmn_vad_state_dict(0)
    return len(pack_fsmn_vad_blob(sd)), lambda: FsmnVad(sd, None, dev), lambda m: m.posteriors([torch.zeros(400).numpy()])     # one frame


@pytest.mark.parametrize("model", [_mf2, _pfenc, _eres2net, _fsmn_vad])
def test_create_forward_close_frees_the_device_memory(model):
    image_bytes, make, forward = model()
    free = []
    for _ in range(3):
        m = make()
        forward(m)
        m.close()
        torch.cuda.synchronize(dev)
        free.append(torch.cuda.mem_get_info(dev)[0])
        m.close()                       # twice: harmless
        assert not m._h                 # the pointer the C-ABI would get is NULL from here on
        del m                           # ... and so is dropping the object afterwards
        gc.collect()
    print(f"{model.__name__}: weight image {image_bytes} B, free after each cycle {free}")
    assert free[0] - free[2] < image_bytes, (free, image_bytes)
