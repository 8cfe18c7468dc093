"""Build libsdeng.so (gfx950) in-tree with hipcc.

    python -m sde_sampler_lrds_amd.build [-j N] [--force]

The simulate kernel is a template over (feature tiles, reference kind, in-loop score kind, update form);
each instantiation is its own translation unit (generated under csrc/gen/) so they compile in parallel.
hipcc cross-compiles for gfx950 without a GPU.
"""
from __future__ import annotations

import argparse
import hashlib
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
GEN = os.path.join(CSRC, "gen")
# experiment knobs: SDENG_OUT = another library path (its objects go to csrc/obj_<name>/), SDENG_PACKED=0/1 below
LIB = os.environ.get("SDENG_OUT") or os.path.join(PKG, "libsdeng.so")
OBJ = os.path.join(CSRC, "obj" if not os.environ.get("SDENG_OUT") else "obj_" + os.path.basename(LIB).split(".")[0])
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -ffp-contract=off: the integrator and log-weight updates must round like the reference's separate
# torch ops (no silent a*b+c fusion); fused multiply-adds are written explicitly where wanted.
FLAGS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fPIC", "-Wno-comment", "-Wno-unused-command-line-argument"]
# Packed fp32 (v_pk_{add,mul,fma}_f32) stays disabled.  With two waves per SIMD the build that uses them is not
# reproducible on MI355X (the pre-empted wave of a SIMD gets wrong values; DESIGN 4a, profiles/r02_packed_fp32_hazard_experiments.log)
# and it is slower anyway (6.11 vs 5.92 ms on cfg 2).  SDENG_PACKED=1 builds that variant for A/B runs only.
PACKED = os.environ.get("SDENG_PACKED", "0") == "1"
if not PACKED:
    FLAGS += ["-Xclang", "-target-feature", "-Xclang", "-packed-fp32-ops"]
if os.environ.get("SDENG_DEFS"):  # experiment knob: extra -D flags (ablation builds)
    FLAGS += ["-D" + d for d in os.environ["SDENG_DEFS"].split()]
if os.environ.get("SDENG_CXXFLAGS"):  # experiment knob: extra compiler flags (e.g. "-mllvm -amdgpu-sched-strategy=iterative-ilp")
    FLAGS += os.environ["SDENG_CXXFLAGS"].split()
if os.environ.get("SDENG_WAVES"):  # experiment knob: waves per workgroup (8 = 2 per SIMD, 4 = 1 per SIMD)
    FLAGS.append("-DSD_WAVES=" + os.environ["SDENG_WAVES"])

DTS = (1, 2, 3, 4, 5, 6, 7, 8)  # feature tiles of 16, NT = ceil(d / 16)
DTS_FULL = (1, 2, 3, 4, 6, 8)    # full-covariance reference: two staged pieces of NT/2 output tiles when NT > 4 (5 and 7 run on 6 and 8)
LIN, EM, EUBO = 0, 1, 3          # SDENG_FORM_*


def _sim(nt, ref, sc, forms):
    """k_simulate instances: PAR 0 (plain), 1 (injected noise / trajectory), and 2 (control perturbation) on the forward forms."""
    return [("sim", nt, (ref, sc, fm, par)) for fm in forms for par in ((0, 1, 2) if fm in (LIN, EM) else (0, 1))]


def _cmcd(nt):
    """k_simulate_cmcd instances: TGT (CT_LOGREG 0, CT_GMM 1, CT_PHI4 2, CT_RINGS 3, CT_ZERO 4) x EUBO x PAR."""
    tgts = [(1, 0), (1, 1), (2, 0)] + ([(0, 0)] if nt <= 4 else []) + ([(3, 0), (3, 1), (4, 0), (4, 1)] if nt == 1 else [])
    return [("cmcd", nt, (tgt, eubo, par)) for tgt, eubo in tgts for par in (0, 1)]


# Every kernel instance, grouped by translation unit (csrc/gen/<unit>.hip): unit -> [(family, NT, template parameters after NT)].
# The units and gen/registry.hip -- the sorted table sdeng_api.hip looks launchers up in -- are both generated from this one list.
# REF: 0 none, 1 Gauss, 2 mixture (K <= 4), 3 larger mixture, 4 full covariance, 5 shared variance on the matrix pipe.
# SC (in-loop score of a Score / Lerp / CancelDrift control): 0 none, 1 mixture / rings, 2 phi^4, 3 logistic regression, 4 the
# full-covariance target held in the reference slot.
UNITS = {
    # (EUBO: every reference-SDE loss -- ClippedCtrl or a score control --, and DIS without a reference)
    **{f"sim_{nt}_{ref}_{sc}": _sim(nt, ref, sc, (LIN, EM) + ((EUBO,) if ref != 0 or sc != 0 else ()))
       for nt in DTS for ref in (0, 1, 2, 3) for sc in (0, 1, 2)},
    **{f"sim_{nt}_0_3": _sim(nt, 0, 3, (LIN, EM)) for nt in (1, 2, 3, 4)},  # logistic-regression design matrix in LDS: d <= 64
    **{f"sim_{nt}_4_0": _sim(nt, 4, 0, (LIN, EM, EUBO)) for nt in DTS_FULL},
    **{f"sim_{nt}_4_{sc}": _sim(nt, 4, sc, (LIN, EM, EUBO)) for nt in DTS_FULL for sc in (1, 2)},  # score control over a full-covariance reference
    **{f"sim_{nt}_4_4": _sim(nt, 4, 4, (LIN, EM)) for nt in DTS_FULL},
    **{f"sim_{nt}_5_0": _sim(nt, 5, 0, (LIN, EM)) for nt in DTS},
    **{f"ctrl_{nt}": [("ctrl", nt, (sc,)) for sc in (0, 1, 2)] for nt in DTS},
    # low-latency small-batch kernels: a tile's features over four waves, d > 64; REF 0..2 x form x PERT
    **{f"split_{nt}": [("split", nt, (ref, fm, pert)) for ref in (0, 1, 2) for fm in (LIN, EM) for pert in (0, 1)] for nt in (5, 6, 7, 8)},
    **{f"cmcd_{nt}": _cmcd(nt) for nt in DTS},
    # drift-net VJP (GX: with the input gradient) and the KL adjoint (SCORE: ADJ_NONE, _GMM, _PHI4, _EXT) share a unit
    **{f"vjp_{nt}": [("vjp", nt, (gx,)) for gx in (1, 0)] + [("adj", nt, (sc,)) for sc in (0, 1, 2, 3)] for nt in DTS},
    "euler_inst": [("euler", nt, (sc,)) for nt in DTS for sc in (0, 1, 2)],  # SDEs without a drift net
    # the CMCD KL adjoint (TGT: CADJ_GMM 1, CADJ_PHI4 2, CADJ_EXT 3 = logistic regression, d <= 64 like its step loop): one unit per
    # instance -- each holds a whole drift-net forward + backward, and a unit of its own keeps the parallel build balanced
    **{f"cadj_{nt}_{tgt}": [("cadj", nt, (tgt,))] for nt in DTS for tgt in (1, 2, 3) if tgt != 3 or nt <= 4},
}
# family -> (header, launcher template, registry enum); the enum order is the registry's sort order (sim_common.hpp)
FAMILIES = {
    "sim": ("sim_kernel.hpp", "launch_simulate", "SD_FAM_SIM"),
    "ctrl": ("sim_kernel.hpp", "launch_ctrl_forward", "SD_FAM_CTRL"),
    "split": ("split_kernel.hpp", "launch_split", "SD_FAM_SPLIT"),
    "euler": ("euler_kernel.hpp", "launch_euler", "SD_FAM_EULER"),
    "cmcd": ("cmcd_kernel.hpp", "launch_cmcd", "SD_FAM_CMCD"),
    "vjp": ("grad_kernel.hpp", "launch_ctrl_vjp", "SD_FAM_VJP"),
    "adj": ("grad_kernel.hpp", "launch_kl_adjoint", "SD_FAM_ADJ"),
    "cadj": ("cmcd_adjoint_kernel.hpp", "launch_cmcd_kl_adjoint", "SD_FAM_CADJ"),
}


def _launcher(fam, nt, params):
    return f"sd_launch_{fam}_{nt}_" + "_".join(map(str, params))


def sources():
    os.makedirs(GEN, exist_ok=True)
    srcs = [os.path.join(CSRC, n) for n in ("sdeng_api.hip", "prep_kernels.hip", "metric_kernels.hip", "cmcd_inst.hip", "tilted_kernel.hip",
                                            "tilted_train_inst.hip", "tilted_moves_inst.hip", "tilted_rds_inst.hip")]
    for unit, insts in UNITS.items():
        headers = sorted({FAMILIES[fam][0] for fam, _, _ in insts})
        body = "".join(f'#include "../{h}"\n' for h in headers) + "".join(
            f"int {_launcher(fam, nt, p)}(const void* a, hipStream_t s) {{ return {FAMILIES[fam][1]}<{nt}, {', '.join(map(str, p))}>(a, s); }}\n"
            for fam, nt, p in insts)
        srcs.append(os.path.join(GEN, unit + ".hip"))
        _write_if_changed(srcs[-1], body)
    order = list(FAMILIES)
    insts = sorted(((order.index(fam), nt, p, fam) for v in UNITS.values() for fam, nt, p in v))
    body = ('// generated by build.py from UNITS: every kernel instance and its launcher, sorted by key (host code only)\n'
            '#include "../sim_common.hpp"\n#ifndef __HIP_DEVICE_COMPILE__\n' +
            "".join(f"int {_launcher(fam, nt, p)}(const void* a, hipStream_t s);\n" for _, nt, p, fam in insts) +
            "constexpr SdKernelEntry sd_registry[] = {\n" +
            "".join(f"    {{sd_key({FAMILIES[fam][2]}, {nt}, {', '.join(map(str, p))}), {_launcher(fam, nt, p)}}},\n" for _, nt, p, fam in insts) +
            "};\nconst int sd_registry_size = sizeof(sd_registry) / sizeof(sd_registry[0]);\n"
            "constexpr bool sd_registry_sorted() {\n  for (int i = 1; i < sizeof(sd_registry) / sizeof(sd_registry[0]); ++i)\n"
            "    if (!(sd_registry[i - 1].key < sd_registry[i].key)) return false;\n  return true;\n}\n"
            'static_assert(sd_registry_sorted(), "registry keys must be unique and sorted (build.py FAMILIES order = SD_FAM_* order)");\n#endif\n')
    srcs.append(os.path.join(GEN, "registry.hip"))
    _write_if_changed(srcs[-1], body)
    return srcs


def _resource_remarks(stderr):
    """-Rpass-analysis=kernel-resource-usage remarks -> [{name, VGPRs, ScratchSize..., Occupancy...}]"""
    import re
    out, cur = [], None
    for line in stderr.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            out.append(cur)
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = int(m.group(2))
    return out


def _write_if_changed(path, body):
    if os.path.exists(path) and open(path).read() == body:
        return
    with open(path, "w") as f:
        f.write(body)


def _digest(with_sources=True):
    """Hash of the flags and the headers (+ the .hip sources): the library stamp, or the part every object depends on."""
    h = hashlib.sha256()
    for root in (CSRC, os.path.join(PKG, "..", "include")):
        for name in sorted(os.listdir(root)):
            if name.endswith((".hpp", ".h") + ((".hip",) if with_sources else ())):
                h.update(open(os.path.join(root, name), "rb").read())
    h.update(" ".join(FLAGS).encode())
    return h.hexdigest()


def build(jobs: int | None = None, force: bool = False, verbose: bool = True) -> str:
    stamp = os.path.join(OBJ, "digest.txt")
    dig = _digest()
    if not force and os.path.exists(LIB) and os.path.exists(stamp) and open(stamp).read() == dig:
        return LIB
    os.makedirs(OBJ, exist_ok=True)
    srcs = sources()
    jobs = jobs or min(8, os.cpu_count() or 1)

    usage = {}
    common = _digest(with_sources=False)

    def compile_one(src):
        """One translation unit -> object; skipped when neither the flags, nor a header, nor this source changed."""
        import json
        obj = os.path.join(OBJ, os.path.basename(src).replace(".hip", ".o"))
        key = hashlib.sha256((common + open(src).read()).encode()).hexdigest()
        meta = obj + ".json"
        if not force and os.path.exists(obj) and os.path.exists(meta):
            m = json.load(open(meta))
            if m.get("key") == key:
                usage[os.path.basename(src)] = m["usage"]
                return obj
        cmd = [HIPCC, *FLAGS, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr}")
        usage[os.path.basename(src)] = _resource_remarks(r.stderr)
        json.dump({"key": key, "usage": usage[os.path.basename(src)]}, open(meta, "w"))
        return obj

    with ThreadPoolExecutor(max_workers=jobs) as ex:
        objs = list(ex.map(compile_one, srcs))
    with open(os.path.join(OBJ, "kernel_resources.txt"), "w") as f:  # registers / scratch / occupancy of every kernel (compiler remarks)
        f.write("# unit kernel VGPRs AGPRs scratch_bytes_per_lane occupancy_waves_per_SIMD LDS_bytes\n")
        for unit in sorted(usage):
            for k in usage[unit]:
                f.write(f"{unit} {k['name']} {k.get('VGPRs', '?')} {k.get('AGPRs', '?')} {k.get('ScratchSize [bytes/lane]', '?')} "
                        f"{k.get('Occupancy [waves/SIMD]', '?')} {k.get('LDS Size [bytes/block]', '?')}\n")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr}")
    with open(stamp, "w") as f:
        f.write(dig)
    if verbose:
        print(f"built {LIB} ({os.path.getsize(LIB) / 1e6:.1f} MB, {len(objs)} objects)")
    return LIB


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-j", type=int, default=None)
    ap.add_argument("--force", action="store_true")
    a = ap.parse_args()
    build(a.j, a.force)
