"""pytest plugin: log every resampling request the suite makes through the package's loader, with the kernel family that served it.

    AAI_REQUEST_LOG=requests.jsonl python -m pytest tests -m gpu -p tools.request_log

One JSON line per call of a resampling entry point of libaai_hip.so: the request as the library saw it (policy bits included),
channels, source type and aai_last_kernel() afterwards.  tools/rot_variants_report.py turns such a log into the list of template
instantiations the logged calls reached.  (Calls a test makes from a child process, or through a loader of its own, are not seen.)
"""
import json
import os

# entry point -> (index of the channels argument or None, index of the AAI_DTYPE_* argument or None)
ENTRIES = {
    "aai_resample_f32": (None, None), "aai_resample_f64": (None, None), "aai_resample_device_f32": (None, None),
    "aai_resample_batch_device_f32": (None, None), "aai_resample_band_device_f32": (None, None),
    "aai_resample_batch_device": (None, 3), "aai_resample_host": (None, 2), "aai_resample_batch_host": (None, 3),
    "aai_resample_interleaved_device": (2, 4), "aai_resample_interleaved_host": (1, 3),
}


def pytest_configure(config):
    path = os.environ.get("AAI_REQUEST_LOG")
    if not path:
        return
    from area_average_interpolation_amd import _lib as L
    lib = L.load()
    out = open(path, "a")
    seen = set()

    def wrap(name, fn, chan_at, dtype_at):
        def call(*args):
            rc = fn(*args)
            rq = args[0]._obj
            rec = {f: getattr(rq, f) for f, _ in L.Request._fields_}
            rec.update(entry=name, channels=int(args[chan_at]) if chan_at is not None else 1,
                       dtype=int(args[dtype_at]) if dtype_at is not None else 0, rc=rc, kernel=lib.aai_last_kernel().decode())
            line = json.dumps(rec, sort_keys=True)
            if line not in seen:
                seen.add(line)
                out.write(line + "\n")
                out.flush()
            return rc
        return call

    for name, (chan_at, dtype_at) in ENTRIES.items():
        setattr(lib, name, wrap(name, getattr(lib, name), chan_at, dtype_at))
