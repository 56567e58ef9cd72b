/*
 * hs_report_device.h — report.hip's host interface: the report program's
 * passes (hs_report_passes.h) on the device, for hs_lit.cpp.
 */
#ifndef VSA_HS_REPORT_DEVICE_H
#define VSA_HS_REPORT_DEVICE_H

#include "hs_report_passes.h"

struct vsa_ctx;

namespace vsa_report {

/* a database's Tables in HBM, uploaded once per (scratch, database);
 * pool_bytes = the size of t.pool */
struct DeviceTables;
int device_tables_create(vsa_ctx *ctx, const Tables &t, uint64_t pool_bytes, DeviceTables **out);
void device_tables_free(DeviceTables *d);

/* a corpus's block table in HBM plus the buffers of the passes, which grow
 * with the records and are kept between runs */
struct DeviceReport;
int device_report_create(vsa_ctx *ctx, const DeviceTables *tabs, const BlockTable &bt,
                         const uint64_t *offsets, const uint64_t *lens, uint32_t nblocks,
                         const uint8_t *d_data, DeviceReport **out);
void device_report_free(DeviceReport *r);
/* the passes over n sorted device records (a completed scan's); counts =
 * host, nblocks, optional.  VSA_OK or a VSA_E_* code */
int device_report_run(DeviceReport *r, const uint64_t *d_keys, const uint32_t *d_ids, uint64_t n,
                      uint64_t *counts, uint64_t *total);
/* the last run's matches: device pointer, valid until the next run */
int device_report_matches(DeviceReport *r, const vsa_hs_match_t **d_matches, uint64_t *n);
/* their first n to the host */
int device_report_copy(DeviceReport *r, vsa_hs_match_t *out, uint64_t n);

} // namespace vsa_report

#endif
