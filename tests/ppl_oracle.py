"""The chain of PPL.distances restated on the CPU oracle, shared by tests/test_gpu_ppl.py and tools/ppl_bench.py so that the
test and the recorded figures of profiles/ppl.txt cannot drift.  No device and no test runner is needed to import it."""
import numpy as np
import torch

RES, FMAP_BASE = 32, 512        # the size of the whole-chain GPU test: skip G, seeded LPIPS weights


def oracle_distances(entries, g_params, l_params, space, crop, epsilon, m, dtype):
    """The chain of PPL.distances restated on the CPU oracle in `dtype`, the recorded draws replayed in the documented order."""
    from oracle import lpips as OL
    from oracle import networks_stylegan2 as ON
    from oracle.misc import lerp, slerp_t
    from inclusivegan_amd.metrics.perceptual_path_length import crop_geometry
    gp = {k: v.to(dtype) for k, v in g_params.items()}
    lpp = {k: v.to(dtype) for k, v in l_params.items()}
    num_layers = int(np.log2(RES)) * 2 - 2
    noise_names = ['G_synthesis/noise%d' % i for i in range(num_layers - 1)]
    per_batch = 2 + len(noise_names)
    assert len(entries) % per_batch == 0
    y0, y1, x0, x1, factor = crop_geometry(RES, RES, crop)
    assert factor == 1
    out = []
    for k in range(len(entries) // per_batch):
        tape = entries[k * per_batch:(k + 1) * per_batch]
        assert [e[0] for e in tape] == ['normal', 'uniform'] + ['normal'] * len(noise_names)
        lat = torch.from_numpy(tape[0][1]).to(dtype)
        t = torch.from_numpy(tape[1][1]).to(dtype)
        assert tuple(lat.shape) == (2 * m, 512) and tuple(t.shape) == (m,)
        for name, (_, noise) in zip(noise_names, tape[2:]):
            assert tuple(noise.shape) == tuple(gp[name].shape)
            gp[name] = torch.from_numpy(noise).to(dtype)
        sc = ON.Scope(gp)
        eps = torch.tensor(epsilon, dtype=dtype)
        if space == 'w':
            dl = ON.G_mapping(sc.sub('G_mapping'), lat, dlatent_broadcast=num_layers)
            a, b, tt = dl[0::2], dl[1::2], t[:, None, None]
            e = torch.stack([lerp(a, b, tt), lerp(a, b, tt + eps)], dim=1).reshape(dl.shape)
        else:
            a, b, tt = lat[0::2], lat[1::2], t[:, None]
            le = torch.stack([slerp_t(a, b, tt), slerp_t(a, b, tt + eps)], dim=1).reshape(lat.shape)
            e = ON.G_mapping(sc.sub('G_mapping'), le, dlatent_broadcast=num_layers)
        img = ON.G_synthesis_stylegan2(sc.sub('G_synthesis'), e, None, resolution=RES, fmap_base=FMAP_BASE, architecture='skip', randomize_noise=False)
        img = (img[:, :, y0:y1, x0:x1] + 1) * (255 / 2)
        out.append(OL.lpips(lpp, img[0::2], img[1::2]) * (1 / epsilon ** 2))
    return torch.cat(out).double().numpy()
