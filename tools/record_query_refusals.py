#!/usr/bin/env python3
"""Every refusal the query entries make before a device is touched, as a table: `cases()` builds the calls, `python3
tools/record_query_refusals.py` runs them against the loaded library (RTRACE_HIP_LIBRARY, or the product) and writes status and message of
each into tests/golden/query_refusals.json.  tests/test_refusals_host.py replays cases() against the built libraries and compares with the
committed table byte for byte: it never regenerates it.  Record the table BEFORE a change to the launch layer, replay it after.

The scene is a stand-in handle, as in tests/test_sweep_host.py: the checks read only the head of rt_scene (csrc/rt_capi.hip) -- precision
at byte 24, n_items at byte 28 -- and every call here is refused before anything else of it is used.  Each case is a call every check
accepts with ONE thing wrong: a NULL argument, n == 0, a bad mode, k or capacity, an output without the list it belongs to, one pointer
misaligned (by 1 byte; by 4 where 8 are needed), or -- host entries -- one value of element 1 of 2 outside the domain."""
import ctypes as C
import json
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from rust_tracer_amd import capi  # noqa: E402

TABLE = os.path.join(ROOT, "tests", "golden", "query_refusals.json")
N, K, CAPACITY, N_ITEMS = 2, 2, 4, 2
NAN, INF = float("nan"), float("inf")

# kinds of parameter: "scene", "mode", "k", "n", "capacity", "margin", "none" (stats, stream), "real" (REAL[]), "word" (32-bit[]),
# "long" (uint64[]).  `!` after a buffer's name: the entry refuses NULL for it.
RAYS_TAIL = "distance_out! normal_out item_out:word"
LISTS = "offsets_out:long total_out!:long stats:none"
ENTRIES = {
    "rt_intersect_rays": "scene mode rays! tmax n %s stats:none" % RAYS_TAIL,
    "rt_intersect_rays_device": "scene mode rays! tmax n %s stream:none stats:none" % RAYS_TAIL,
    "rt_intersect_rays_ordered": "scene mode rays! tmax n order:word %s stats:none" % RAYS_TAIL,
    "rt_intersect_rays_ordered_device": "scene mode rays! tmax n order:word %s stream:none stats:none" % RAYS_TAIL,
    "rt_intersect_rays_multi": "scene mode k rays! tmax n %s hits_out:word stats:none" % RAYS_TAIL,
    "rt_intersect_rays_multi_device": "scene mode k rays! tmax n %s hits_out:word stream:none stats:none" % RAYS_TAIL,
    "rt_intersect_rays_multi_ordered": "scene mode k rays! tmax n order:word %s hits_out:word stats:none" % RAYS_TAIL,
    "rt_intersect_rays_multi_ordered_device": "scene mode k rays! tmax n order:word %s hits_out:word stream:none stats:none" % RAYS_TAIL,
    "rt_trace_rays": "scene rays! n color_out! alpha_out stats:none",
    "rt_trace_rays_device": "scene rays! n color_out! alpha_out stream:none stats:none",
    "rt_trace_rays_ordered": "scene rays! n order:word color_out! alpha_out stats:none",
    "rt_trace_rays_ordered_device": "scene rays! n order:word color_out! alpha_out stream:none stats:none",
    "rt_ray_order": "scene rays! n order_out!:word",
    "rt_ray_order_device": "scene rays! n order_out!:word stream:none",
    "rt_near_spheres": "scene mode k points! radius n exclude:word order:word gap_out! item_out:word found_out:word stats:none",
    "rt_sweep_spheres": "scene mode rays! radius tmax n exclude:word order:word distance_out! normal_out item_out:word stats:none",
    "rt_scene_contacts": "scene margin capacity pairs_out:word gap_out " + LISTS,
    "rt_overlap_spheres": "scene queries! n margin exclude:word order:word capacity items_out:word gap_out " + LISTS,
    "rt_scene_impacts": "scene disp! capacity pairs_out:word time_out " + LISTS,
    "rt_swept_overlaps": "scene queries! qdisp! n disp exclude:word order:word capacity items_out:word time_out normal_out " + LISTS,
    "rt_first_contacts": "scene mode queries! qdisp! n disp exclude:word order:word time_out! item_out:word normal_out stats:none",
}
for _name in ("rt_near_spheres", "rt_sweep_spheres", "rt_scene_contacts", "rt_overlap_spheres", "rt_scene_impacts", "rt_swept_overlaps", "rt_first_contacts"):
    ENTRIES[_name + "_device"] = ENTRIES[_name] + " stream:none"

MAX_K = {"rt_intersect_rays_multi": capi.RT_MULTIHIT_MAX_K, "rt_near_spheres": capi.RT_NEAR_MAX_K}
# an output given without the list it belongs to: the arguments to pass as NULL
WITHOUT = {"rt_scene_contacts": [("pairs_out",)], "rt_scene_impacts": [("pairs_out",)], "rt_overlap_spheres": [("items_out",)],
           "rt_swept_overlaps": [("items_out",), ("items_out", "time_out")]}
# element 1 of 2 of the host entries' inputs: what every element holds, and per component the values outside the domain
GOOD = {"rays": (0, 0, 0, 0, 0, 1), "tmax": (1,), "radius": (0.5,), "points": (0, 0, 0), "queries": (0, 0, 0, 0.5), "qdisp": (0, 0, 0), "disp": (0, 0, 0)}
OUTSIDE = (("nan", NAN), ("inf", INF), ("3e15", 3e15))
BAD_RADIUS = (("negative", -1.0), ("nan", NAN), ("2e15", 2e15))
BAD = {"rays": [(1, OUTSIDE), (4, (("dir_nan", NAN), ("dir_2", 2.0)))], "tmax": [(0, (("nan", NAN),))], "radius": [(0, BAD_RADIUS)],
       "points": [(1, OUTSIDE)], "queries": [(1, OUTSIDE), (3, BAD_RADIUS)], "qdisp": [(1, OUTSIDE)], "disp": [(1, OUTSIDE)]}
NEAR_RADIUS = [(0, (("nan", NAN),))]             # (rt_near_spheres takes any radius that is a number)


def _params(entry):
    out = []
    for word in ENTRIES[entry].split():
        name, _, kind = word.partition(":")
        required = name.endswith("!")
        name = name.rstrip("!")
        out.append((name, kind or (name if name in ("scene", "mode", "k", "n", "capacity", "margin") else "real"), required))
    return out


def _stand_in(precision):
    buf = C.create_string_buffer(4096)
    struct.pack_into("<iI", buf, 24, precision, N_ITEMS)
    return buf


def _buffer(name, kind, precision):
    """64 elements of 8 bytes: room for every size these calls name.  Inputs hold values inside the domain."""
    R = C.c_float if precision == capi.RT_F32 else C.c_double
    if kind == "long":
        return (C.c_uint64 * 64)()
    if kind == "word":
        return (C.c_uint32 * 128)(0, 1) if name == "order" else (C.c_int32 * 128)(*([-1] * 128))
    return (R * (512 // C.sizeof(R)))(*(GOOD.get(name, (0,)) * 2))


class Case:
    def __init__(self, entry, precision, label, change):
        self.id = "%s/%s/%s" % (entry, "f32" if precision == capi.RT_F32 else "f64", label)
        self.entry, self.precision, self.change = entry, precision, change

    def run(self, lib):
        """(status, message) of the call on `lib`, a ctypes.CDLL of the library"""
        keep = {"scene": _stand_in(self.precision)}
        value = {"scene": C.addressof(keep["scene"]), "mode": 0, "k": K, "n": N, "capacity": CAPACITY, "margin": 0.0}
        for name, kind, _ in _params(self.entry):
            if kind in ("real", "word", "long"):
                keep[name] = _buffer(name, kind, self.precision)
                value[name] = C.addressof(keep[name])
            elif kind == "none":
                value[name] = None
        self.change(value, keep)
        f = getattr(lib, self.entry)
        f.argtypes, f.restype = getattr(capi.lib, self.entry).argtypes, C.c_int
        lib.rt_last_error_message.restype = C.c_char_p
        status = f(*[value[name] for name, _, _ in _params(self.entry)])
        return int(status), lib.rt_last_error_message().decode()


def _set(**kw):
    return lambda value, keep: value.update(kw)


def _shift(name, by):
    return lambda value, keep: value.update({name: value[name] + by})


def _poke(name, index, x):
    def change(value, keep):
        keep[name][index] = x
    return change


def cases():
    for entry in sorted(ENTRIES):
        params = _params(entry)
        names = [p[0] for p in params]
        base = entry[:-len("_device")] if entry.endswith("_device") else entry
        host = base == entry
        for precision in (capi.RT_F32, capi.RT_F64):
            def case(label, change):
                return Case(entry, precision, label, change)
            yield case("null_scene", _set(scene=None))
            for name, kind, required in params:
                if required:
                    yield case("null_" + name, _set(**{name: None}))
            if "n" in names:
                yield case("n_0", _set(n=0))
            if "mode" in names:
                for mode in (2, -1):
                    yield case("mode_%d" % mode, _set(mode=mode))
            if "k" in names:
                for k in (0, MAX_K[base.replace("_ordered", "")] + 1):
                    yield case("k_%d" % k, _set(k=k))
            if "capacity" in names:
                yield case("capacity_2^31", _set(capacity=1 << 31))
            if "margin" in names:
                yield case("margin_nan", _set(margin=NAN))
            for gone in WITHOUT.get(base, ()):
                yield case("without_" + "_".join(gone), _set(**{name: None for name in gone}))
            for name, kind, _ in params:
                if kind in ("real", "word", "long"):
                    yield case("misaligned_" + name, _shift(name, 1))
                    if kind == "long" or (kind == "real" and precision == capi.RT_F64):
                        yield case("misaligned_by_4_" + name, _shift(name, 4))
            if not host:
                continue
            for name, kind, _ in params:
                bad = NEAR_RADIUS if (base, name) == ("rt_near_spheres", "radius") else BAD.get(name, ())
                for component, values in bad:
                    for label, x in values:
                        yield case("%s_1_%d_%s" % (name, component, label), _poke(name, len(GOOD[name]) + component, x))
                if name == "order":
                    for order in ((0, 0), (0, 2)):
                        yield case("order_%d_%d" % order, _poke("order", 1, order[1]))


def main():
    lib = C.CDLL(capi.LIB_PATH)
    table = {}
    for c in cases():
        assert c.id not in table, c.id
        status, message = c.run(lib)
        # a call that is not refused would go on to use the stand-in as a scene: such a case must not reach the table
        assert status == capi.RT_ERR_INVALID_ARGUMENT and message, (c.id, status, message)
        if c.precision == capi.RT_F64 and "misaligned_by_4" in c.id:
            assert message.endswith("8-byte aligned"), (c.id, message)
        table[c.id] = [status, message]
    with open(TABLE, "w") as f:
        f.write("{\n%s\n}\n" % ",\n".join("%s: %s" % (json.dumps(k), json.dumps(table[k])) for k in sorted(table)))
    print("%d refusals of %s -> %s" % (len(table), capi.LIB_PATH, os.path.relpath(TABLE, ROOT)))


if __name__ == "__main__":
    main()
