#!/usr/bin/env python3
"""Register / scratch / occupancy guard of the stencil kernels (round-3 review, item 3).

The build (tmlqcd_amd/csrc/Makefile) compiles every .hip file with -Rpass-analysis=kernel-resource-usage and keeps the
compiler's remarks next to the object (lib/<name>.ru.txt).  This script parses them, writes the table
(profiles/r04_resource_usage.txt) and FAILS the build when an instance the default dispatch of hopping_impl.inc can launch
spills (scratch > 0) or drops below three waves per SIMD -- the split path once lost 40 % to a spill nobody looked at
(profiles/r03_split_forms.md, last paragraph of `split_early`).

    check_resources.py [--table OUT.txt] lib/linalg.ru.txt lib/bicgstab.ru.txt lib/eig.ru.txt lib/laph.ru.txt lib/hopping.ru.txt lib/hopping32.ru.txt lib/clover.ru.txt lib/gauge.ru.txt lib/flow.ru.txt lib/meas.ru.txt lib/rational.ru.txt lib/nd.ru.txt lib/nd32.ru.txt lib/poly.ru.txt
"""
import re
import subprocess
import sys

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")
CXXFILT = "c++filt"

# Instances the default dispatch reaches (launch_variant / launch_exterior / launch_pack in hopping_impl.inc), as regular
# expressions on the demangled name, with the floor each must keep.  Template arguments of hop_kernel:
#   <EPI, TSKIP, NTIO, BS, MINW, GAUX, STG>
# EPI 5 / 6 / 7 / 10 / 11 / 13 are the clover epilogues (a 6x6 block product per chirality on top of the stencil, up to 256 VGPRs + a few
# AGPRs) and TSKIP 2 is the per-lane form of ragged test lattices: those are held to "no scratch"; everything else to "no scratch" and
# three waves per SIMD.
CLOVER_EPI = {5, 6, 7, 10, 11, 13}
RULES = [
    # fp64, large lattices: the LDS-staged kernel, __launch_bounds__(256, 3) for the twisted-mass epilogues, (256, 1) for the clover ones
    (r"^void hop64::hop_kernel<(\d+), ([013]), true, 256, (3|1), -1, 64>", "fp64 staged"),
    # ... and its packed link read (GAUX 15, "gauge_pack"): twisted-mass epilogues of unsplit lattices, three waves per SIMD, no scratch
    (r"^void hop64::hop_kernel<(\d+), 0, true, 256, 3, 15, 64>", "fp64 staged packed"),
    # ... and the 104-byte form of it (GAUX 16, "gauge_pack_compact"): the same eight epilogues, the same floor
    (r"^void hop64::hop_kernel<(\d+), 0, true, 256, 3, 16, 64>", "fp64 staged packed 104"),
    # the shifted residual epilogue of the multi-shift CG (EPI 12, mms.hip) in the gather kernel: one more field than its sibling EPI 9
    # (190 VGPRs, two waves per SIMD); its staged form above keeps three
    (r"^void hop64::hop_kernel<12, 0, true, (64|256), 1, (-1|-2), 0>", "fp64 gather shifted res", 2),
    # fp64, small lattices and ragged shapes: the gather kernel
    (r"^void hop64::hop_kernel<(\d+), ([0123]), true, (64|256), (1|3), (-1|-2), 0>", "fp64 gather"),
    (r"^void hop64::hop_split4_kernel<(\d+), true>", "fp64 hop-split"),
    (r"^void hop64::hop_exterior_kernel<(\d+), true>", "fp64 exterior"),
    (r"^void hop64::pack_faces_kernel", "fp64 pack"),
    # fp32: gather kernel by default ("lds32" 0), the staged one behind the option
    (r"^void hop32::hop_kernel<(\d+), ([0123]), true, (64|256), 1, (-1|-2), 0>", "fp32 gather"),
    (r"^void hop32::hop_exterior_kernel<(\d+), true>", "fp32 exterior"),
    (r"^void hop32::pack_faces_kernel", "fp32 pack"),
    # the two plaquette-leaf kernels of the clover rows (interior instances): 230 - 254 VGPRs by design, two waves per SIMD, no scratch
    (r"^void sw_term_kernel<SwFastLd>", "sw_term", 2),
    (r"^void sw_all_gather_kernel<SwFastLd>", "sw_all gather", 2),
    # the gauge monomial (gauge.hip): four to five 3x3 complex matrices live per link, no scratch, two waves per SIMD
    (r"^void gaugehip::gauge_force_kernel<(true|false)>", "gauge force", 2),
    (r"^(void )?gaugehip::(plaquette|rectangle)_sum_kernel", "gauge action", 2),
    # the gradient flow (flow.hip): a stage is the plaquette force's staple sum plus the Cayley-Hamilton exponential; the field strength
    # keeps two projected leaves of a site next to one rolled path product: no scratch, two waves per SIMD
    (r"^void flowhip::flow_stage_kernel<[012]>", "flow stage", 2),
    (r"^(void )?flowhip::field_strength_kernel", "field strength", 2),
    # the online measurements (meas.hip): the slice sums hold one spinor and up to six accumulators, the Polyakov line three matrices, the
    # oriented plaquettes the four of plaquette_sum_kernel and six sums: no scratch, two waves per SIMD, the final pass included
    (r"^(void )?meaship::\w+_kernel", "online measurements", 2),
    # the batched hopping force of the rational monomials (rational.hip): no scratch, two waves per SIMD
    (r"^(void )?rathip::deriv_Sb_batch_kernel", "batched hopping force", 2),
    # the clover doublet (nd.hip): the doublet stencil with the clover mixing as its epilogue, and the site-local form of the same
    # epilogues -- two 6x6 block products per flavour and chirality, streamed one 3x3 block at a time: no scratch, two waves per SIMD
    (r"^void ndsw_hop_kernel<(\d+), (64|256), (true|false)>", "clover doublet stencil", 2),
    (r"^void ndsw_mix_kernel<(\d+)>", "clover doublet site-local", 2),
    # the fp32 doublet (nd32.hip): the doublet stencil on float2 arithmetic with the mixing as its epilogue -- no scratch and the gather
    # kernels' three waves per SIMD -- and the site-local mixing kernel, a stream of eight fields
    (r"^void nd32_hop_kernel<(\d+), (64|256), (true|false)>", "fp32 doublet stencil", 3),
    (r"^void nd32_mix_kernel<(\d+)>", "fp32 doublet site-local", 3),
    # the vector part of mixed_cg_mms_tm_nd (nd32.hip): streams of float4 planes: no scratch, eight waves per SIMD; the pass over x and d
    # holds the twelve loads of two planes in flight per lane and keeps six
    (r"^(void )?mms32_(r|addp)_kernel", "fp32 multi-shift streams", 8),
    (r"^(void )?mms32_xd_kernel", "fp32 multi-shift x and d pass", 6),
    (r"^(void )?sw_invert_nd_kernel", "sw_invert_nd", 2),
    (r"^(void )?sw_deriv_nd_kernel", "sw_deriv_nd", 2),
    # the batched clover outer products of the rational forces: one wave per block n of swm / swp, 36 doubles of accumulators
    (r"^(void )?sw_spinor_eo_batch_kernel", "batched sw_spinor_eo", 3),
    # the tr-log energies: a fully unrolled 6x6 factorisation per site in registers
    (r"^void sw_trace_kernel<(true|false)>", "sw_trace / sw_trace_nd", 2),
    # the complex linalg of the chronological guess (linalg.hip), one instance per group size: the accumulators of a group stay in
    # registers -- no scratch -- at the eight waves per SIMD the build reports for dotr_kernel
    (r"^void csg_dot_kernel<\d+>", "batched scalar_prod", 8),
    (r"^void csg_axpy_kernel<\d+>", "batched assign_diff_mul", 8),
    (r"^void csg_lincomb_kernel<\d+, (true|false)>", "lincomb", 8),
    # the two streams of the correction monomials (linalg.hip): one accumulator per thread whatever np is, and the subtraction with
    # the block sums of sqnorm_kernel: no scratch, eight waves per SIMD
    (r"^(void )?rat_sum_kernel", "rat_sum", 8),
    (r"^(void )?diff_sqnorm_kernel", "diff_sqnorm", 8),
    # BiCGstab (linalg.hip, bicgstab.hip): the two three-field singles and the five fused kernels between the two stencils of an
    # iteration -- K4 walks six fields with three accumulators --: streams like the ones above, no scratch, eight waves per SIMD
    (r"^void cplx3_kernel<[01]>", "three-field complex singles", 8),
    (r"^(void )?bicghip::(dot_kernel<(true|false)>|sub_kernel|update_kernel|dir_kernel)", "fused BiCGstab", 8),
    # the eigensolver (eig.hip): its dots, projection, scaling and Chebyshev step are streams like the ones above -- four elements of w
    # in registers whatever the number of basis vectors -- no scratch, eight waves per SIMD.  The rotation keeps K complex accumulators
    # per thread, K = 8 / 16 / 32 / 64 by the number of columns: no scratch; the floor of each instance is what the build reports for
    # this, the only form that was built (a column-group form for large k was not, so 64 columns at one wave per SIMD is unrivalled, not best)
    (r"^(void )?eighip::(eig_dots_kernel|eig_project_kernel|eig_scale_kernel|eig_cheb_kernel)", "eigensolver streams", 8),
    (r"^void eighip::basis_rotate_kernel<8>", "basis rotation, 8 columns", 8),
    (r"^void eighip::basis_rotate_kernel<16>", "basis rotation, 16 columns", 6),
    (r"^void eighip::basis_rotate_kernel<32>", "basis rotation, 32 columns", 3),
    (r"^void eighip::basis_rotate_kernel<64>", "basis rotation, 64 columns", 1),
    # the LapH eigensystem (laph.hip): the 3D Laplacian on colour vectors holds one link and two colour vectors per site -- no scratch,
    # the stencils' three waves per SIMD in all three forms; its dots, projection, scaling and combination are the streams of eig.hip with
    # a slice dimension -- no scratch, eight waves per SIMD; the final pass, the fill and the layout
    # change hold a handful of registers: eight waves as well.  The rotation parks its n inputs in LDS (n x 512 bytes per one-wave block: at
    # n = 24 that alone admits three waves per SIMD) and keeps 16 real accumulators next to a row of Y in scalar registers: no scratch,
    # four waves per SIMD is more than its LDS ever lets in
    (r"^void laphhip::laph_kernel<[012]>", "3D Laplacian", 3),
    (r"^(void )?laphhip::(laph_dots_kernel|laph_project_kernel|laph_scale_kernel|laph_comb_kernel)", "LapH streams", 8),
    (r"^(void )?laphhip::(laph_final_kernel|laph_fill_kernel)", "LapH final pass, fill", 8),
    (r"^(void )?laphhip::laph_rotate_kernel", "LapH rotation", 4),
    (r"^void laphhip::cv_layout_kernel<(true|false)>", "colour-vector layout", 8),
    # the four-term combination of the polynomial monomial (poly.hip), both flavours of a doublet per launch: a stream like the ones above
    (r"^(void )?polyhip::comb4_kernel", "four-term combination", 8),
    # propagator / source records (spinor_io.hip): byte work through an LDS tile, a handful of registers; "no scratch" is the floor
    (r"^void spinor_io_kernel<[24], (true|false)>", "spinor record pack / unpack", 1),
]


def parse(path):
    out = []
    cur = None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"mangled": m.group(1), "file": path}
            out.append(cur)
            continue
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2)) if m.group(2).lstrip("-").isdigit() else m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run([CXXFILT], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True)
        return r.stdout.split("\n")[: len(names)]
    except (OSError, subprocess.CalledProcessError):
        return names


def main(argv):
    table = None
    files = []
    it = iter(argv)
    for a in it:
        if a == "--table":
            table = next(it)
        else:
            files.append(a)
    if not files:
        print(__doc__)
        return 2
    ks = []
    for f in files:
        ks += parse(f)
    for k, n in zip(ks, demangle([k["mangled"] for k in ks])):
        k["name"] = re.sub(r"\(.*$", "", n.replace("(anonymous namespace)::", ""))   # drop the parameter list
    bad, rows, guarded = [], [], 0
    for k in sorted(ks, key=lambda k: k["name"]):
        tag, floor = "", None
        for rule in RULES:
            rx, what = rule[0], rule[1]
            m = re.match(rx, k["name"])
            if m and len(rule) > 2:
                floor = rule[2]
                tag = "%s (>= %d waves)" % (what, floor)
                break
            if m:
                g = m.groups()
                epi = int(g[0]) if g else -1
                ragged = len(g) > 1 and g[1] == "2"
                floor = 1 if (epi in CLOVER_EPI or ragged) else 3
                # the one-kernel form of the direct carrier sizes its wait budget on two waves per SIMD for the clover epilogues (direct_one_kernel)
                if epi in CLOVER_EPI and len(g) > 1 and g[1] == "3":
                    floor = 2
                tag = "%s (>= %d waves)" % (what, floor)
                break
        scratch, occ = k.get("ScratchSize [bytes/lane]", -1), k.get("Occupancy [waves/SIMD]", -1)
        verdict = ""
        if floor is not None:
            guarded += 1
            if scratch != 0 or occ < floor:
                verdict = "FAIL"
                bad.append(k)
            else:
                verdict = "ok"
        rows.append("%-96s %5s %5s %7s %4s %7s  %-28s %s" % (k["name"][:96], k.get("VGPRs", "?"), k.get("AGPRs", "?"), scratch, occ,
                                                          k.get("LDS Size [bytes/block]", "?"), tag, verdict))
    head = "%-96s %5s %5s %7s %4s %7s  %-28s %s" % ("kernel", "VGPR", "AGPR", "scratch", "occ", "LDS", "guard", "")
    text = "\n".join([head, "-" * len(head)] + rows) + "\n"
    text += "\n%d kernels, %d guarded, %d failing\n" % (len(ks), guarded, len(bad))
    if table:
        with open(table, "w") as f:
            f.write("# -Rpass-analysis=kernel-resource-usage of the stencil translation units, gfx950 (tools/check_resources.py;\n"
                    "# written by every build: tmlqcd_amd/csrc/Makefile).  guard = an instance the default dispatch can launch.\n")
            f.write(text)
    if guarded == 0:
        print("check_resources: no guarded kernel found in", files, file=sys.stderr)
        return 1
    if bad:
        print(text)
        print("check_resources: %d default-dispatch kernel(s) spill or run below their occupancy floor:" % len(bad), file=sys.stderr)
        for k in bad:
            print("   %s: scratch %s B/lane, %s waves/SIMD, %s VGPRs" % (k["name"], k.get("ScratchSize [bytes/lane]"), k.get("Occupancy [waves/SIMD]"), k.get("VGPRs")), file=sys.stderr)
        return 1
    print("check_resources: %d kernels, %d guarded, all within budget" % (len(ks), guarded))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
