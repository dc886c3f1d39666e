// rbg_capi.hip -- the C-ABI of include/rbg.h: owns the host copy of the flat index and its
// HBM replica, stages host batches, launches the kernels of k_search.hip / k_locate.hip / k_markers.hip / k_build.hip.
// There is deliberately no CPU compute path in this library.
#include <hip/hip_runtime.h>
#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>

#include <map>

#include "../../include/rbg.h"
#include "rbg_dev.h"
#include "rbg_jump.h"
#include "rbg_docdir.hpp"
#include "rbg_fl.hpp"
#include "rbg_isa.hpp"
#include "rbg_sam.hpp"
#include "rbg_host.hpp"


// The C-ABI of include/rbg.h, by concern (one translation unit: the parts share the scratch pools, the options and the handle's definition in an
// anonymous namespace, and the kernels' launchers are declared once in rbg_dev.h):
#include "capi/core.ipp"          // the handle, options, pools, arena
#include "capi/upload_runs.ipp"   // run-indexed layout: tables on the device, composition of the k-mer depths
#include "capi/query.ipp"         // what every query entry point shares: staging of a host batch, the result pool, the big copies, ragged_finish
#include "capi/load.ipp"          // upload() and its budget / layout rules; load / convert / build entry points; info
#include "capi/device_api.ipp"    // *_dev entry points
#include "capi/hostpath.ipp"      // host-pointer entry points, micro-batching
#include "capi/text.ipp"          // rbg_align_text
#include "capi/seeds.ipp"         // markers, marker seeds (the shared seed pass: greedy or lmem, plan and fill), greedy seeding
#include "capi/tally.ipp"         // the marker tally: per-marker counts of the report's lines, accumulated on the device (rbg_markers_tally: report.ipp)
#include "capi/report.ipp"        // rb_markers' report on the device, pass by pass: strands, the seed pass, canonical records, selection; records, text or tally
#include "capi/loc_markers.ipp"   // the text-position marker table, markers at located positions (rb_locs' path)
#include "capi/docs.ipp"          // the document table on the device, documents of located positions (rbg_doc_hits*, rbg_resolve_offsets_dev*)
#include "capi/fl.ipp"            // the FL index on the device (rbg_fl_prepare), FL of rows, the right extension of located seeds (fl_extend.hip)
#include "capi/extract.ipp"       // the ISA sample on the device (rbg_extract_prepare), rows of text positions, the text of intervals (extract.hip)
#include "capi/build_text.ipp"    // an index from its text: suffix array, runs and samples on the device (sa_build.hip), rbg_build_from_text, rbg_convert_text
#include "capi/sam.ipp"           // rbg_align_sam: SAM lines of raw reads, both strands, written on the device; rbg_sam_header
#include "capi/replicas.ipp"      // replicas in one process, counters, RCCL
