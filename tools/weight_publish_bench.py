#!/usr/bin/env python3
"""Cost of a weight refresh of a live net, host route against device route, on one GPU.

Per net shape (20 blocks x 256 filters and 6 blocks x 64 filters, 15x15), one warm-up load and the median of
--loads timed loads of each route, all in one process:

  host blob     az_net_load_weights on a numpy blob that is already on the host
  host route    what a trainer on the same GPU had to do before: state_dict -> one float32 tensor -> .cpu() ->
                numpy -> az_net_load_weights
  device route  az_amd.state_dict_blob (a device tensor) -> HipNeuralNetwork.load_weights_device; wall time of
                the whole route and of the load alone, and the device time of the pack launches (HIP events,
                az_diag_net_pack_ms with az_net_profile on)

Bytes written are the payload of the net's weight pool plus the device copy of the blob, from
az_diag_device_mem around the first load; the store rate is those bytes over the pack launches' device
time, set against the 8 TB/s HBM peak and the 6.29 TB/s a float4 copy reaches.  Needs a GPU; prints a
table and one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "alphazero-multi-game_amd"), os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)

import numpy as np   # noqa: E402
import torch         # noqa: E402  (before libaz_hip.so: one HIP runtime)

import az_amd                    # noqa: E402
from az_amd import _lib          # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def device_mem():
    b, k = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.check(_lib.lib().az_diag_device_mem(ctypes.byref(b), ctypes.byref(k)))
    return b.value


def state_dict_like(desc, blob):
    """The blob cut into a state_dict's tensors on the device (a trainer's parameters and BN buffers)."""
    import net_oracle
    sd, off = {}, 0
    t = torch.from_numpy(blob).cuda()
    for name, shape, _, _ in net_oracle.param_shapes(desc):
        n = int(np.prod(shape))
        sd[name] = t[off:off + n].reshape(shape).clone()
        off += n
        if name.endswith("running_var"):
            sd[name[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(1, device="cuda")
    return sd


def timed(fn, loads):
    fn()                                        # warm-up
    out = []
    for _ in range(loads):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def measure(eng, blocks, channels, precision, loads):
    import net_oracle
    desc = az_amd.gomoku_net_desc(board_size=15, channels=channels, blocks=blocks, precision=precision, max_batch=8)
    blob = net_oracle.init_blob(desc, 11)
    sd = state_dict_like(desc, blob)
    res = {"net": f"{blocks}b x {channels}f", "params": int(blob.size)}
    # host routes
    net = az_amd.HipNeuralNetwork(eng, desc)
    res["host_blob_ms"] = timed(lambda: net.load_weights(blob), loads)

    def host_route():
        flat = torch.cat([v.reshape(-1).float() for k, v in sd.items() if not k.endswith("num_batches_tracked")])
        net.load_weights(flat.cpu().numpy())
    res["host_route_ms"] = timed(host_route, loads)
    ref = net.forward(np.zeros((2, 11, 15, 15), np.float32))
    net.close()
    # device route
    net = az_amd.HipNeuralNetwork(eng, desc)
    m0 = device_mem()
    out = az_amd.state_dict_blob(sd)
    net.load_weights_device(out)
    res["bytes_written"] = device_mem() - m0       # the weight pool and the net's copy of the blob (`out` is torch's)
    net.profile(True)
    pack = []

    def device_load():
        net.load_weights_device(out)
        ms = ctypes.c_double(0)
        _lib.check(_lib.lib().az_diag_net_pack_ms(net.h, ctypes.byref(ms)))
        pack.append(ms.value)
    res["device_load_ms"] = timed(device_load, loads)
    res["pack_ms"] = (statistics.median(pack[1:]), min(pack[1:]), max(pack[1:]))
    net.profile(False)

    def device_route():
        az_amd.state_dict_blob(sd, out=out)
        net.load_weights_device(out)
    res["device_route_ms"] = timed(device_route, loads)
    got = net.forward(np.zeros((2, 11, 15, 15), np.float32))
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]), "the two routes' nets differ"
    assert np.array_equal(net.get_weights(), blob)
    net.close()
    res["store_bytes_per_s"] = res["bytes_written"] / (res["pack_ms"][0] * 1e-3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--loads", type=int, default=5)
    args = ap.parse_args()
    eng = az_amd.Engine(0)
    rows = [measure(eng, 20, 256, az_amd.AZ_PREC_FP16, args.loads), measure(eng, 6, 64, az_amd.AZ_PREC_FP16, args.loads)]
    print(f"device: {eng.device_name}; median (min .. max) of {args.loads} loads after one warm-up, milliseconds")
    for r in rows:
        print(f"\n{r['net']} at 15x15: {r['params']} parameters, {r['bytes_written'] / 1e6:.1f} MB of weight buffers written per load")
        for key, label in (("host_blob_ms", "az_net_load_weights, blob on the host"),
                           ("host_route_ms", "host route: state_dict -> cpu -> load"),
                           ("device_route_ms", "device route: state_dict_blob -> load_weights_device"),
                           ("device_load_ms", "  load_weights_device alone (wall)"),
                           ("pack_ms", "  its pack launches (HIP events)")):
            md, lo, hi = r[key]
            print(f"  {label:58s} {md:9.3f}  ({lo:.3f} .. {hi:.3f})")
        bw = r["store_bytes_per_s"]
        print(f"  store rate of the pack launches: {bw / 1e9:.0f} GB/s = {100 * bw / HBM_PEAK:.1f}% of the 8 TB/s HBM peak, "
              f"{100 * bw / HBM_COPY:.1f}% of a float4 copy's 6.29 TB/s")
        print(f"  device route / host route: {r['host_route_ms'][0] / r['device_route_ms'][0]:.1f}x faster")
    print(json.dumps({"weight_publish": rows}))


if __name__ == "__main__":
    main()
